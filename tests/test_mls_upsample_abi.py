"""CPU-side checks of the upsampling entries (ope_mls_upsample, ope_mls_upsample_cloud and their helpers): declared, exported and bound;
the ctypes structs lay out exactly as the C compiler lays out ope_mls_upsample_params / ope_mls_upsample_stats; the defaults are
pcl::MovingLeastSquares' own; the smoothing entries' structs are untouched and the ABI version stays 5."""
import ctypes
import os
import re
import subprocess

import pytest

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


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "ope.h"
#define O(t, tag, m) printf("%s.%s %zu\n", tag, #m, offsetof(t, m))
int main(void) {
  printf("sizeof_p %zu\nsizeof_s %zu\nsizeof_smooth %zu\n", sizeof(ope_mls_upsample_params), sizeof(ope_mls_upsample_stats), sizeof(ope_mls_params));
  O(ope_mls_upsample_params, "p", radius); O(ope_mls_upsample_params, "p", polynomial_fit); O(ope_mls_upsample_params, "p", order);
  O(ope_mls_upsample_params, "p", sqr_gauss_param); O(ope_mls_upsample_params, "p", compute_normals);
  O(ope_mls_upsample_params, "p", voxel_size); O(ope_mls_upsample_params, "p", dilation_iterations);
  O(ope_mls_upsample_stats, "s", n_in); O(ope_mls_upsample_stats, "s", n_valid); O(ope_mls_upsample_stats, "s", n_voxels);
  O(ope_mls_upsample_stats, "s", n_invalid_nearest); O(ope_mls_upsample_stats, "s", n_polynomial);
  O(ope_mls_upsample_stats, "s", n_rejected_farther); O(ope_mls_upsample_stats, "s", n_out); O(ope_mls_upsample_stats, "s", data_size);
  O(ope_mls_upsample_stats, "s", launches); O(ope_mls_upsample_stats, "s", host_syncs);
  printf("abi %d\n", OPE_ABI_VERSION);
  return 0;
}
"""


def test_upsample_layouts_match_the_c_compiler(ope, tmp_path):
    c = tmp_path / "probe.c"
    c.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.check_call(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)], text=True).splitlines()
    want = {ln.split(" ", 1)[0]: ln.split(" ", 1)[1] for ln in lines}
    structs = {"p": ope.MlsUpsampleParams, "s": ope.MlsUpsampleStats}
    got = {"sizeof_" + t: str(ctypes.sizeof(S)) for t, S in structs.items()}
    got["sizeof_smooth"] = str(ctypes.sizeof(ope.MlsParams))   # untouched
    for t, S in structs.items():
        for name, _ in S._fields_:
            got[t + "." + name] = str(getattr(S, name).offset)
    got["abi"] = "5"   # the change only adds to the ABI
    assert got == want


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
