"""The façade over ope_color_filter: ope::ProcessingPcd::getFilterRgb (compat::ConditionalRemoval with setKeepOrganized(true)) on an
organised 16 x 12 cloud returns the input's size, width and height, every passing point untouched and every failing point with
its colour and x = y = z = NaN; the unorganised form returns the finite passing points in order.  Exact, against a numpy mask."""
import importlib
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_pkg

pytestmark = pytest.mark.gpu

pcd = importlib.import_module("object-pose-estimation_amd.pcd")
LIB = os.path.join(ROOT, "object-pose-estimation_amd")
W, H = 16, 12

CHECK = r'''
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "ope/pcd_io.hpp"
#include "ope/processing_pcd.hpp"
namespace pcl = ope::compat;
static void dump(const char *tag, const pcl::PointCloud<pcl::PointXYZRGB> &c) {
  std::printf("%s %zu %u %u %d\n", tag, c.size(), c.width, c.height, c.is_dense ? 1 : 0);
  for (const auto &p : c.points) {
    unsigned u[4];
    std::memcpy(u, &p.x, 12);
    std::memcpy(u + 3, &p.rgb, 4);
    std::printf("%08x %08x %08x %08x\n", u[0], u[1], u[2], u[3]);
  }
}
int main(int argc, char **argv) {
  pcl::PointCloud<pcl::PointXYZRGB>::Ptr in(new pcl::PointCloud<pcl::PointXYZRGB>);
  if (argc < 10 || pcl::io::loadPCDFile(argv[1], *in) != 0) return 3;
  in->width = (unsigned)std::atoi(argv[2]);
  in->height = (unsigned)std::atoi(argv[3]);
  int v[6];
  for (int k = 0; k < 6; ++k) v[k] = std::atoi(argv[4 + k]);
  ope::ProcessingPcd proc;
  dump("getFilterRgb", *proc.getFilterRgb(in, v[0], v[1], v[2], v[3], v[4], v[5]));
  typedef pcl::PackedRGBComparison<pcl::PointXYZRGB> Cmp;
  pcl::ConditionAnd<pcl::PointXYZRGB>::Ptr cond(new pcl::ConditionAnd<pcl::PointXYZRGB>());
  cond->addComparison(Cmp::Ptr(new Cmp("g", pcl::ComparisonOps::GT, v[2])));
  pcl::ConditionalRemoval<pcl::PointXYZRGB> rem(cond);
  rem.setInputCloud(in);
  pcl::PointCloud<pcl::PointXYZRGB> out;
  rem.filter(out);
  dump("unorganized", out);
  return 0;
}
'''


def hexrow(p, c):
    return " ".join("%08x" % int(v) for v in list(np.asarray(p, np.float32).view(np.uint32)) + [c])


@pytest.mark.parametrize("limits", [(40, 200, 30, 220, 10, 250), (-1, 256, -1, 256, -1, 256), (100, 101, 0, 255, 0, 255)], ids=["some", "all", "none"])
def test_get_filter_rgb_keeps_the_cloud_organised(limits, tmp_path):
    load_pkg().build_library()
    n = W * H
    rng = np.random.default_rng(21)
    pts = rng.uniform(-0.5, 0.5, (n, 3)).astype(np.float32)
    if limits[0] >= 0:                      # (the case that keeps every point runs on a dense cloud: is_dense stays true)
        pts[[5, 77, 150], 1] = np.nan
    rgb = rng.integers(0, 1 << 24, n).astype(np.uint32)
    r, g, b = (rgb >> 16) & 255, (rgb >> 8) & 255, rgb & 255
    src, exe, cloud = tmp_path / "check.cpp", str(tmp_path / "check"), str(tmp_path / "in.pcd")
    src.write_text(CHECK)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe, "-L", LIB, "-lope_hip",
                           "-Wl,-rpath," + LIB, "-Wl,-rpath,/opt/rocm/lib"])
    pcd.write_pcd(cloud, pts, rgb)
    run = subprocess.run([exe, cloud, str(W), str(H), *[str(v) for v in limits]], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    keep = (r > limits[0]) & (r < limits[1]) & (g > limits[2]) & (g < limits[3]) & (b > limits[4]) & (b < limits[5])
    print("[getFilterRgb] keeps %d of %d" % (keep.sum(), n))
    nan3 = np.full(3, np.nan, np.float32)
    fin = np.isfinite(pts).all(1)
    want = ["getFilterRgb %d %d %d %d" % (n, W, H, 1 if keep.all() and fin.all() else 0)]
    want += [hexrow(pts[i] if keep[i] else nan3, rgb[i]) for i in range(n)]
    sel = np.flatnonzero((g > limits[2]) & fin)
    want += ["unorganized %d %d 1 1" % (len(sel), len(sel))] + [hexrow(pts[i], rgb[i]) for i in sel]
    got = run.stdout.splitlines()
    # a NaN written by the filter and one read from the file may differ in their payload bits: compare NaN as NaN
    def norm(line):
        w = line.split()
        return " ".join("nan" if len(x) == 8 and k < 3 and (int(x, 16) & 0x7fffffff) > 0x7f800000 else x for k, x in enumerate(w))
    assert [norm(x) for x in got[1:]] == [norm(x) for x in want[1:]]
    assert got[0] == want[0]
