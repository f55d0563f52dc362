"""CPU-side checks of the peel's entries (ope_plane_peel, ope_peel_default_params): declared, exported and bound; the header
compiles as C; the ctypes structs lay out exactly as the C compiler lays out ope_peel_params / ope_peel_result; the default is
the reference's literal (objectsegmentationplane.cpp:300)."""
import ctypes
import os
import re
import subprocess

import pytest

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


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "ope.h"
#define O(t, tag, m) printf("%s.%s %zu\n", tag, #m, offsetof(t, m))
int main(void) {
  printf("sizeof_p %zu\nsizeof_r %zu\n", sizeof(ope_peel_params), sizeof(ope_peel_result));
  O(ope_peel_params, "p", keep_fraction); O(ope_peel_params, "p", max_planes);
  O(ope_peel_result, "r", n_planes); O(ope_peel_result, "r", n_rest); O(ope_peel_result, "r", stop);
  O(ope_peel_result, "r", launches); O(ope_peel_result, "r", host_syncs);
  printf("abi %d\nstop %d %d %d\n", OPE_ABI_VERSION, OPE_PEEL_FRACTION, OPE_PEEL_NO_INLIERS, OPE_PEEL_MAX_PLANES);
  return 0;
}
"""


def test_peel_layouts_match_the_c_compiler(ope, tmp_path):
    c = tmp_path / "probe.c"
    c.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)], text=True).splitlines()
    want = {ln.split(" ", 1)[0]: ln.split(" ", 1)[1] for ln in lines}
    structs = {"p": ope.PeelParams, "r": ope.PeelResult}
    got = {"sizeof_" + t: str(ctypes.sizeof(S)) for t, S in structs.items()}
    for t, S in structs.items():
        for name, _ in S._fields_:
            got[t + "." + name] = str(getattr(S, name).offset)
    got["abi"] = "5"   # the change only adds to the ABI
    got["stop"] = "%d %d %d" % (ope.PEEL_FRACTION, ope.PEEL_NO_INLIERS, ope.PEEL_MAX_PLANES)
    assert got == want and got["stop"] == "0 1 2"


def test_peel_defaults_are_the_reference_literals(ope):
    p = ope.PeelParams(-1.0, -1)
    ctypes.CDLL(ope.LIB_PATH).ope_peel_default_params(ctypes.byref(p))
    assert p.keep_fraction == 0.3      # objectsegmentationplane.cpp:300
    assert p.max_planes == 0           # the reference has no cap
