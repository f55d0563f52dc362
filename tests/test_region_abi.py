"""CPU-side checks of region growing (ope_region_grow, ope_region_grow_cloud): declared, exported and bound; the ctypes structs lay
out exactly as the C compiler lays out ope_region_params / ope_region_stats; the defaults are the reference's literals
(segmentationregiongrow.cpp:25-36)."""
import ctypes
import math
import os
import re

import pytest

from abi_probe import c_layout, ctypes_layout
from conftest import ROOT, load_pkg

HEADER = os.path.join(ROOT, "include", "ope.h")
ENTRIES = ("ope_region_default_params", "ope_region_grow", "ope_region_grow_cloud", "ope_region_last_stats")


@pytest.fixture(scope="module")
def ope():
    pkg = load_pkg()
    pkg.build_library()
    return pkg


@pytest.mark.parametrize("name", ENTRIES)
def test_region_entry_is_declared_exported_and_bound(ope, name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\b(int|void)\s+" + name + r"\s*\(", src)
    assert hasattr(ctypes.CDLL(ope.LIB_PATH), name)
    assert name in {n for n, _, _ in ope.ABI}


def test_region_layouts_match_the_c_compiler(ope):
    structs = {ope.RegionParams: "ope_region_params", ope.RegionStats: "ope_region_stats"}
    assert ctypes_layout(structs) == c_layout(structs)


def test_region_binding_has_the_header_s_argument_counts(ope):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    table = {n: a for n, _, a in ope.ABI}
    for name in ENTRIES:
        args = re.search(r"\b" + name + r"\s*\(([^)]*)\)", src).group(1)
        assert len(args.split(",")) == len(table[name]), name


def test_region_defaults_are_the_reference_literals(ope):
    p = ope.default_region_params()
    assert p.number_of_neighbours == 15                       # setNumberOfNeighbours (15) (segmentationregiongrow.cpp:31)
    assert p.normals_k == 30                                  # setKSearch (30) (:25)
    assert p.smoothness_threshold == 10.0 / 180.0 * math.pi   # setSmoothnessThreshold (10.0 / 180.0 * M_PI) (:35)
    assert p.curvature_threshold == 1.0                       # setCurvatureThreshold (1.0) (:36)
    assert (p.min_size, p.max_size) == (500, 1000000)         # setMinClusterSize (500), setMaxClusterSize (1000000) (:28-29)
    assert ope.default_region_params(min_size=1).min_size == 1
