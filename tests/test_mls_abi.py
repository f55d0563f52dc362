"""CPU-side checks of the moving-least-squares entries (ope_mls_smooth, ope_mls_smooth_cloud and their helpers): declared, exported and
bound; the ctypes structs lay out exactly as the C compiler lays out ope_mls_params / ope_mls_stats; the defaults are
pcl::MovingLeastSquares' own with ProcessingPcd::getSmooth's polynomial fit; the ABI version stays 5."""
import ctypes
import os
import re
import subprocess

import pytest

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


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "ope.h"
#define O(t, tag, m) printf("%s.%s %zu\n", tag, #m, offsetof(t, m))
int main(void) {
  printf("sizeof_p %zu\nsizeof_s %zu\n", sizeof(ope_mls_params), sizeof(ope_mls_stats));
  O(ope_mls_params, "p", radius); O(ope_mls_params, "p", polynomial_fit); O(ope_mls_params, "p", order);
  O(ope_mls_params, "p", sqr_gauss_param); O(ope_mls_params, "p", compute_normals);
  O(ope_mls_stats, "s", n_in); O(ope_mls_stats, "s", n_out); O(ope_mls_stats, "s", n_plane_only); O(ope_mls_stats, "s", n_dropped);
  O(ope_mls_stats, "s", neighbours_total);
  printf("abi %d\n", OPE_ABI_VERSION);
  return 0;
}
"""


def test_mls_layouts_match_the_c_compiler(ope, tmp_path):
    c = tmp_path / "probe.c"
    c.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.check_call(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)], text=True).splitlines()
    want = {ln.split(" ", 1)[0]: ln.split(" ", 1)[1] for ln in lines}
    structs = {"p": ope.MlsParams, "s": ope.MlsStats}
    got = {"sizeof_" + t: str(ctypes.sizeof(S)) for t, S in structs.items()}
    for t, S in structs.items():
        for name, _ in S._fields_:
            got[t + "." + name] = str(getattr(S, name).offset)
    got["abi"] = "5"   # the change only adds to the ABI
    assert got == want


def test_mls_defaults(ope):
    p = ope.default_mls_params()
    assert p.radius == 0.0              # MovingLeastSquares: search_radius_ (0); the caller sets it (getSmooth's argument)
    assert p.polynomial_fit == 1        # processingpcd.cpp: setPolynomialFit (true)
    assert p.order == 2                 # MovingLeastSquares: order_ (2)
    assert p.sqr_gauss_param == 0.0     # 0: radius^2 (setSearchRadius)
    assert p.compute_normals == 0       # MovingLeastSquares: compute_normals_ (false)
    assert ope.default_mls_params(radius=0.02, order=1).order == 1
    assert ope.lib().ope_abi_version() == 5
