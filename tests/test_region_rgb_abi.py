"""CPU-side checks of colour-based region growing (ope_region_grow_rgb, ope_region_grow_rgb_cloud) and the colour filter
(ope_color_filter, ope_color_filter_cloud): declared, exported and bound; the ctypes structs lay out exactly as the C compiler lays
out ope_region_rgb_params / ope_region_rgb_stats; the defaults are the reference's literals (segmentationregiongrow.cpp:97-106)."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT, load_pkg

HEADER = os.path.join(ROOT, "include", "ope.h")
ENTRIES = ("ope_region_rgb_default_params", "ope_region_grow_rgb", "ope_region_grow_rgb_cloud", "ope_region_rgb_last_stats", "ope_color_filter",
           "ope_color_filter_cloud")


@pytest.fixture(scope="module")
def ope():
    pkg = load_pkg()
    pkg.build_library()
    return pkg


@pytest.mark.parametrize("name", ENTRIES)
def test_region_rgb_entry_is_declared_exported_and_bound(ope, name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\b(int|void)\s+" + name + r"\s*\(", src)
    assert hasattr(ctypes.CDLL(ope.LIB_PATH), name)
    assert name in {n for n, _, _ in ope.ABI}


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "ope.h"
#define O(t, tag, m) printf("%s.%s %zu\n", tag, #m, offsetof(t, m))
int main(void) {
  printf("sizeof_p %zu\nsizeof_s %zu\n", sizeof(ope_region_rgb_params), sizeof(ope_region_rgb_stats));
  O(ope_region_rgb_params, "p", region_neighbour_number); O(ope_region_rgb_params, "p", distance_threshold);
  O(ope_region_rgb_params, "p", point_color_threshold); O(ope_region_rgb_params, "p", region_color_threshold);
  O(ope_region_rgb_params, "p", min_size); O(ope_region_rgb_params, "p", max_size);
  O(ope_region_rgb_stats, "s", launches); O(ope_region_rgb_stats, "s", host_syncs); O(ope_region_rgb_stats, "s", sweeps);
  O(ope_region_rgb_stats, "s", one_way_edges); O(ope_region_rgb_stats, "s", segments); O(ope_region_rgb_stats, "s", segment_pairs);
  O(ope_region_rgb_stats, "s", homogeneous_regions); O(ope_region_rgb_stats, "s", regions_absorbed);
  O(ope_region_rgb_stats, "s", regions_before_size_filter);
  return 0;
}
"""


def test_region_rgb_layouts_match_the_c_compiler(ope, tmp_path):
    c = tmp_path / "probe.c"
    c.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.check_call(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    want = dict(line.rsplit(" ", 1) for line in subprocess.check_output([str(exe)], text=True).splitlines())
    want = {k: int(v) for k, v in want.items()}
    structs = {"p": ope.RegionRgbParams, "s": ope.RegionRgbStats}
    got = {"sizeof_" + t: ctypes.sizeof(S) for t, S in structs.items()}
    for t, S in structs.items():
        for name, _ in S._fields_:
            got[t + "." + name] = getattr(S, name).offset
    assert got == want


def test_region_rgb_binding_has_the_header_s_argument_counts(ope):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    table = {n: a for n, _, a in ope.ABI}
    for name in ENTRIES:
        args = re.search(r"\b" + name + r"\s*\(([^)]*)\)", src).group(1)
        assert len(args.split(",")) == len(table[name]), name


def test_region_rgb_defaults_are_the_reference_literals(ope):
    p = ope.default_region_rgb_params()
    assert p.region_neighbour_number == 100                 # PCL's region_neighbour_number_, never changed by the reference
    assert p.distance_threshold == 0.1                      # setDistanceThreshold (0.1) (segmentationregiongrow.cpp:100)
    assert p.point_color_threshold == 10.0                  # setPointColorThreshold (10) (:101)
    assert p.region_color_threshold == 10.0                 # setRegionColorThreshold (10) (:102)
    assert (p.min_size, p.max_size) == (700, 2 ** 31 - 1)   # setMinClusterSize (700) (:103); PCL's default maximum
    assert ope.default_region_rgb_params(min_size=1).min_size == 1
    assert ctypes.CDLL(ope.LIB_PATH).ope_abi_version() == 5
