"""CPU-side checks of the upsampling entries (ope_mls_upsample, ope_mls_upsample_cloud and their helpers): declared, exported and bound;
the ctypes structs lay out exactly as the C compiler lays out ope_mls_upsample_params / ope_mls_upsample_stats; the defaults are
pcl::MovingLeastSquares' own; the smoothing entries' structs are untouched and the ABI version stays 5."""
import ctypes
import os
import re

import pytest

from abi_probe import c_layout, ctypes_layout
from conftest import ROOT, load_pkg

HEADER = os.path.join(ROOT, "include", "ope.h")
ENTRIES = ("ope_mls_upsample_default_params", "ope_mls_upsample", "ope_mls_upsample_cloud", "ope_mls_upsample_last_stats")


@pytest.fixture(scope="module")
def ope():
    pkg = load_pkg()
    pkg.build_library()
    return pkg


@pytest.mark.parametrize("name", ENTRIES)
def test_upsample_entry_is_declared_exported_and_bound(ope, name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\b(int|void)\s+" + name + r"\s*\(", src)
    assert hasattr(ctypes.CDLL(ope.LIB_PATH), name)
    assert name in {n for n, _, _ in ope.ABI}
    for method in ("mls_upsample", "mls_upsample_stats"):
        assert callable(getattr(ope.Context, method))


def test_every_upsample_symbol_of_the_header_is_in_the_binding_table(ope):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(ope_mls_upsample\w*)\s*\(", src))
    assert declared == set(ENTRIES)
    assert declared <= {n for n, _, _ in ope.ABI}


def test_upsample_layouts_match_the_c_compiler(ope):
    structs = {ope.MlsUpsampleParams: "ope_mls_upsample_params", ope.MlsUpsampleStats: "ope_mls_upsample_stats",
               ope.MlsParams: "ope_mls_params"}   # the last one untouched
    got = ctypes_layout(structs)
    got["abi"] = 5   # the change only adds to the ABI
    assert got == c_layout(structs, extra={"abi": "OPE_ABI_VERSION"})


def test_upsample_defaults(ope):
    p = ope.default_mls_upsample_params()
    assert p.radius == 0.0                # MovingLeastSquares: search_radius_ (0); the caller sets it (generateMesh: 0.03)
    assert p.polynomial_fit == 1          # regmeshpcd.cpp: setPolynomialFit (true)
    assert p.order == 2                   # MovingLeastSquares: order_ (2); generateMesh sets 4
    assert p.sqr_gauss_param == 0.0       # 0: radius^2 (setSearchRadius)
    assert p.compute_normals == 0         # MovingLeastSquares: compute_normals_ (false)
    assert p.voxel_size == 1.0            # MovingLeastSquares: voxel_size_ (1.0)
    assert p.dilation_iterations == 0     # MovingLeastSquares: dilation_iteration_num_ (0)
    q = ope.default_mls_upsample_params(radius=0.03, order=4, voxel_size=0.002, dilation_iterations=1)
    assert (q.order, q.dilation_iterations) == (4, 1) and abs(q.voxel_size - 0.002) < 1e-9
    with pytest.raises(AttributeError):
        ope.default_mls_upsample_params(upsampling="none")
    assert ope.lib().ope_abi_version() == 5
