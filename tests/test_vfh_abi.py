"""CPU-side checks of the recognition entry points (ope_vfh_*): declared, exported and bound; the ctypes structs lay out exactly
as the C compiler lays out ope_vfh_params / ope_vfh_stats; the defaults are the reference's (objectdetection.cpp:17, PCL's
VFHEstimation constructor); the ABI version stays 5."""
import ctypes
import os
import re

import pytest

from abi_probe import c_layout, ctypes_layout
from conftest import ROOT, load_pkg

HEADER = os.path.join(ROOT, "include", "ope.h")
ENTRIES = ("ope_vfh_default_params", "ope_vfh_batch", "ope_vfh_last_stats", "ope_vfh_db_create", "ope_vfh_db_free", "ope_vfh_db_size",
           "ope_vfh_match", "ope_vfh_recognise")


@pytest.fixture(scope="module")
def ope():
    pkg = load_pkg()
    pkg.build_library()
    return pkg


@pytest.mark.parametrize("name", ENTRIES)
def test_vfh_entry_is_declared_exported_and_bound(ope, name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\b(int|void|size_t)\s+" + name + r"\s*\(", src)
    assert hasattr(ctypes.CDLL(ope.LIB_PATH), name)
    assert name in {n for n, _, _ in ope.ABI}


def test_vfh_layouts_match_the_c_compiler(ope):
    structs = {ope.VfhParams: "ope_vfh_params", ope.VfhStats: "ope_vfh_stats"}
    assert ctypes_layout(structs) == c_layout(structs)


def test_vfh_binding_has_the_header_s_argument_counts(ope):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    table = {n: a for n, _, a in ope.ABI}
    for name in ENTRIES:
        args = re.search(r"\b" + name + r"\s*\(([^)]*)\)", src).group(1)
        assert len(args.split(",")) == len(table[name]), name


def test_vfh_defaults(ope):
    p = ope.default_vfh_params()
    assert p.normals_k == 30                               # normEst.setKSearch (30) (objectdetection.cpp:17)
    assert list(p.viewpoint) == [0.0, 0.0, 0.0]            # vpx_ = vpy_ = vpz_ = 0
    assert (p.use_given_centroid, p.use_given_normal) == (0, 0)
    assert list(p.centroid) == [0.0, 0.0, 0.0] and list(p.normal) == [0.0, 0.0, 0.0]
    q = ope.default_vfh_params(use_given_centroid=1, centroid=(1, 2, 3))
    assert q.use_given_centroid == 1 and list(q.centroid) == [1.0, 2.0, 3.0]


def test_vfh_leaves_the_abi_version_alone(ope):
    assert ope.lib().ope_abi_version() == 5
    for name in ("vfh", "vfh_db", "vfh_match", "vfh_recognise", "vfh_stats"):
        assert callable(getattr(ope.Context, name))
