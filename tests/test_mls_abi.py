"""CPU-side checks of the moving-least-squares entries (ope_mls_smooth, ope_mls_smooth_cloud and their helpers): declared, exported and
bound; the ctypes structs lay out exactly as the C compiler lays out ope_mls_params / ope_mls_stats; the defaults are
pcl::MovingLeastSquares' own with ProcessingPcd::getSmooth's polynomial fit; the ABI version stays 5."""
import ctypes
import os
import re

import pytest

from abi_probe import c_layout, ctypes_layout
from conftest import ROOT, load_pkg

HEADER = os.path.join(ROOT, "include", "ope.h")
ENTRIES = ("ope_mls_default_params", "ope_mls_smooth", "ope_mls_smooth_cloud", "ope_mls_last_stats", "ope_cloud_download_normals")


@pytest.fixture(scope="module")
def ope():
    pkg = load_pkg()
    pkg.build_library()
    return pkg


@pytest.mark.parametrize("name", ENTRIES)
def test_mls_entry_is_declared_exported_and_bound(ope, name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\b(int|void)\s+" + name + r"\s*\(", src)
    assert hasattr(ctypes.CDLL(ope.LIB_PATH), name)
    assert name in {n for n, _, _ in ope.ABI}
    for method in ("mls_smooth", "mls_stats"):
        assert callable(getattr(ope.Context, method))


def test_mls_layouts_match_the_c_compiler(ope):
    structs = {ope.MlsParams: "ope_mls_params", ope.MlsStats: "ope_mls_stats"}
    got = ctypes_layout(structs)
    got["abi"] = 5   # the change only adds to the ABI
    assert got == c_layout(structs, extra={"abi": "OPE_ABI_VERSION"})


def test_mls_defaults(ope):
    p = ope.default_mls_params()
    assert p.radius == 0.0              # MovingLeastSquares: search_radius_ (0); the caller sets it (getSmooth's argument)
    assert p.polynomial_fit == 1        # processingpcd.cpp: setPolynomialFit (true)
    assert p.order == 2                 # MovingLeastSquares: order_ (2)
    assert p.sqr_gauss_param == 0.0     # 0: radius^2 (setSearchRadius)
    assert p.compute_normals == 0       # MovingLeastSquares: compute_normals_ (false)
    assert ope.default_mls_params(radius=0.02, order=1).order == 1
    assert ope.lib().ope_abi_version() == 5
