"""CPU-side checks of colour-based region growing (ope_region_grow_rgb, ope_region_grow_rgb_cloud) and the colour filter
(ope_color_filter, ope_color_filter_cloud): declared, exported and bound; the ctypes structs lay out exactly as the C compiler lays
out ope_region_rgb_params / ope_region_rgb_stats; the defaults are the reference's literals (segmentationregiongrow.cpp:97-106)."""
import ctypes
import os
import re

import pytest

from abi_probe import c_layout, ctypes_layout
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


def test_region_rgb_layouts_match_the_c_compiler(ope):
    structs = {ope.RegionRgbParams: "ope_region_rgb_params", ope.RegionRgbStats: "ope_region_rgb_stats"}
    assert ctypes_layout(structs) == c_layout(structs)


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
