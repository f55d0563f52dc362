"""CPU-side checks of the colour filter (ope_color_filter, ope_color_filter_cloud): declared, exported and bound with the header's
argument counts, the ABI version unchanged, and the façade over them (compat::ConditionalRemoval / ConditionAnd /
PackedRGBComparison, ope::ProcessingPcd::getFilterRgb) compiles as C++17 with warnings on."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT, load_pkg

HEADER = os.path.join(ROOT, "include", "ope.h")
ENTRIES = ("ope_color_filter", "ope_color_filter_cloud")


@pytest.fixture(scope="module")
def ope():
    pkg = load_pkg()
    pkg.build_library()
    return pkg


def header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


@pytest.mark.parametrize("name", ENTRIES)
def test_color_filter_entry_is_declared_exported_and_bound(ope, name):
    assert re.search(r"\bint\s+" + name + r"\s*\(", header())
    assert hasattr(ctypes.CDLL(ope.LIB_PATH), name)
    assert name in {n for n, _, _ in ope.ABI}
    assert ctypes.CDLL(ope.LIB_PATH).ope_abi_version() == 5


def test_color_filter_binding_has_the_header_s_arguments(ope):
    table = {n: a for n, _, a in ope.ABI}
    i32p, vp = ctypes.POINTER(ctypes.c_int32), ctypes.c_void_p
    for name in ENTRIES:
        args = [a.strip() for a in re.search(r"\b" + name + r"\s*\(([^)]*)\)", header()).group(1).split(",")]
        assert len(args) == len(table[name]), name
        # the limits are int32 triples, as the reference's int arguments are; lo before hi
        assert args[2] == "const int32_t lo[3]" and args[3] == "const int32_t hi[3]"
        assert table[name][2] is i32p and table[name][3] is i32p
    assert table["ope_color_filter_cloud"][4]._type_ is vp


def test_color_filter_refuses_null_arguments_without_a_device(ope):
    L = ctypes.CDLL(ope.LIB_PATH)
    n = ctypes.c_size_t(7)
    assert L.ope_color_filter(None, None, None, None, None, ctypes.byref(n)) == ope.OPE_EINVAL
    assert L.ope_color_filter_cloud(None, None, None, None, None, None, ctypes.byref(n)) == ope.OPE_EINVAL


FACADE = r'''
#include "ope/processing_pcd.hpp"
int main() {
  ope::ProcessingPcd proc;
  ope::ProcessingPcd::Cloud::Ptr (ope::ProcessingPcd::*f)(ope::ProcessingPcd::Cloud::Ptr, int, int, int, int, int, int) = &ope::ProcessingPcd::getFilterRgb;
  (void)f; (void)proc;
  // the conjunction as open integer intervals: a fractional limit rounds towards the side that keeps the comparison's truth
  typedef ope::compat::PackedRGBComparison<ope::PointTProc> Cmp;
  ope::compat::ConditionAnd<ope::PointTProc> c;
  c.addComparison(Cmp::Ptr(new Cmp("r", ope::compat::ComparisonOps::GT, 10.5)));
  c.addComparison(Cmp::Ptr(new Cmp("r", ope::compat::ComparisonOps::LT, 20.5)));
  c.addComparison(Cmp::Ptr(new Cmp("g", ope::compat::ComparisonOps::GT, -40)));
  c.addComparison(Cmp::Ptr(new Cmp("b", ope::compat::ComparisonOps::LT, 1000)));
  c.addComparison(Cmp::Ptr(new Cmp("b", ope::compat::ComparisonOps::LT, 7)));
  c.addComparison(Cmp::Ptr(new Cmp("b", ope::compat::ComparisonOps::LT, 9)));
  const int want_lo[3] = {10, -1, -1}, want_hi[3] = {21, 256, 7};
  for (int k = 0; k < 3; ++k)
    if (c.lo_[k] != want_lo[k] || c.hi_[k] != want_hi[k]) return 1;
  return c.isCapable() ? 0 : 2;
}
'''


def test_facade_compiles_and_folds_comparisons_into_intervals(ope, tmp_path):
    src, exe = tmp_path / "f.cpp", str(tmp_path / "f")
    src.write_text(FACADE)
    lib = os.path.dirname(ope.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe, "-L", lib, "-lope_hip",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    assert subprocess.run([exe], timeout=60).returncode == 0
