"""CPU-side checks of the table-top segmentation entries (ope_plane_segment, ope_prism_extract, ope_tabletop_segment and their
helpers): declared, exported and bound; the ctypes structs lay out exactly as the C compiler lays out ope_plane_params /
ope_plane_stats / ope_tabletop_result; the defaults are the reference's literals (objectsegmentationplane.cpp:39-43) and
pcl::SACSegmentation's own."""
import ctypes
import os
import re

import pytest

from abi_probe import c_layout, ctypes_layout
from conftest import ROOT, load_pkg

HEADER = os.path.join(ROOT, "include", "ope.h")
ENTRIES = ("ope_plane_default_params", "ope_plane_segment", "ope_plane_last_stats", "ope_plane_last_hypotheses", "ope_prism_extract",
           "ope_tabletop_segment")


@pytest.fixture(scope="module")
def ope():
    pkg = load_pkg()
    pkg.build_library()
    return pkg


@pytest.mark.parametrize("name", ENTRIES)
def test_plane_entry_is_declared_exported_and_bound(ope, name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\b(int|void)\s+" + name + r"\s*\(", src)
    assert hasattr(ctypes.CDLL(ope.LIB_PATH), name)
    assert name in {n for n, _, _ in ope.ABI}
    for method in ("plane_segment", "prism_extract", "tabletop_segment"):
        assert callable(getattr(ope.Context, method))


def test_plane_layouts_match_the_c_compiler(ope):
    structs = {ope.PlaneParams: "ope_plane_params", ope.PlaneStats: "ope_plane_stats", ope.TabletopResult: "ope_tabletop_result"}
    got = ctypes_layout(structs)
    got["abi"] = 5   # the change only adds to the ABI
    got["status.ok"], got["status.first"], got["status.second"] = ope.TABLETOP_OK, ope.TABLETOP_NO_PLANE_FIRST, ope.TABLETOP_NO_PLANE_SECOND
    got["maxit"] = 1023
    assert got == c_layout(structs, extra={"abi": "OPE_ABI_VERSION", "status.ok": "OPE_TABLETOP_OK",
                                           "status.first": "OPE_TABLETOP_NO_PLANE_FIRST", "status.second": "OPE_TABLETOP_NO_PLANE_SECOND",
                                           "maxit": "OPE_PLANE_MAX_ITERATIONS"})


def test_plane_defaults_are_the_reference_literals(ope):
    p = ope.default_plane_params()
    assert p.distance_threshold == 0.01      # setDistanceThreshold (0.01) (objectsegmentationplane.cpp:43)
    assert p.max_iterations == 50            # SACSegmentation: max_iterations_ (50)
    assert p.probability == 0.99             # SACSegmentation: probability_ (0.99)
    assert p.optimize_coefficients == 1      # setOptimizeCoefficients (true) (:39)
    assert p.seed == 12345                   # SampleConsensusModel: rng_alg_.seed (12345u) when random is false
    assert ope.default_plane_params(seed=7).seed == 7
