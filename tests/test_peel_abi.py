"""CPU-side checks of the peel's entries (ope_plane_peel, ope_peel_default_params): declared, exported and bound; the header
compiles as C; the ctypes structs lay out exactly as the C compiler lays out ope_peel_params / ope_peel_result; the default is
the reference's literal (objectsegmentationplane.cpp:300)."""
import ctypes
import os
import re

import pytest

from abi_probe import c_layout, ctypes_layout
from conftest import ROOT, load_pkg

HEADER = os.path.join(ROOT, "include", "ope.h")
ENTRIES = ("ope_peel_default_params", "ope_plane_peel")


@pytest.fixture(scope="module")
def ope():
    pkg = load_pkg()
    pkg.build_library()
    return pkg


@pytest.mark.parametrize("name", ENTRIES)
def test_peel_entry_is_declared_exported_and_bound(ope, name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\b(int|void)\s+" + name + r"\s*\(", src)
    assert hasattr(ctypes.CDLL(ope.LIB_PATH), name)
    assert name in {n for n, _, _ in ope.ABI}
    for method in ("plane_peel", "except_plane_segment"):
        assert callable(getattr(ope.Context, method))


def test_peel_layouts_match_the_c_compiler(ope):
    structs = {ope.PeelParams: "ope_peel_params", ope.PeelResult: "ope_peel_result"}
    got = ctypes_layout(structs)
    got["abi"] = 5   # the change only adds to the ABI
    got["stop.fraction"], got["stop.no_inliers"], got["stop.max_planes"] = stop = (ope.PEEL_FRACTION, ope.PEEL_NO_INLIERS, ope.PEEL_MAX_PLANES)
    assert got == c_layout(structs, extra={"abi": "OPE_ABI_VERSION", "stop.fraction": "OPE_PEEL_FRACTION",
                                           "stop.no_inliers": "OPE_PEEL_NO_INLIERS", "stop.max_planes": "OPE_PEEL_MAX_PLANES"})
    assert stop == (0, 1, 2)


def test_peel_defaults_are_the_reference_literals(ope):
    p = ope.PeelParams(-1.0, -1)
    ctypes.CDLL(ope.LIB_PATH).ope_peel_default_params(ctypes.byref(p))
    assert p.keep_fraction == 0.3      # objectsegmentationplane.cpp:300
    assert p.max_planes == 0           # the reference has no cap
