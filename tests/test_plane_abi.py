"""CPU-side checks of the table-top segmentation entries (ope_plane_segment, ope_prism_extract, ope_tabletop_segment and their
helpers): declared, exported and bound; the ctypes structs lay out exactly as the C compiler lays out ope_plane_params /
ope_plane_stats / ope_tabletop_result; the defaults are the reference's literals (objectsegmentationplane.cpp:39-43) and
pcl::SACSegmentation's own."""
import ctypes
import os
import re
import subprocess

import pytest

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


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "ope.h"
#define O(t, tag, m) printf("%s.%s %zu\n", tag, #m, offsetof(t, m))
int main(void) {
  printf("sizeof_p %zu\nsizeof_s %zu\nsizeof_t %zu\n", sizeof(ope_plane_params), sizeof(ope_plane_stats), sizeof(ope_tabletop_result));
  O(ope_plane_params, "p", distance_threshold); O(ope_plane_params, "p", probability); O(ope_plane_params, "p", max_iterations);
  O(ope_plane_params, "p", optimize_coefficients); O(ope_plane_params, "p", seed);
  O(ope_plane_stats, "s", iterations); O(ope_plane_stats, "s", hypotheses); O(ope_plane_stats, "s", launches);
  O(ope_plane_stats, "s", host_syncs); O(ope_plane_stats, "s", best); O(ope_plane_stats, "s", found);
  O(ope_tabletop_result, "t", status); O(ope_tabletop_result, "t", n_prism); O(ope_tabletop_result, "t", n_plane);
  O(ope_tabletop_result, "t", n_not_plane); O(ope_tabletop_result, "t", coeff_first); O(ope_tabletop_result, "t", coeff_second);
  O(ope_tabletop_result, "t", corners); O(ope_tabletop_result, "t", iterations_first); O(ope_tabletop_result, "t", iterations_second);
  O(ope_tabletop_result, "t", launches); O(ope_tabletop_result, "t", host_syncs);
  printf("abi %d\nstatus %d %d %d\nmaxit %d\n", OPE_ABI_VERSION, OPE_TABLETOP_OK, OPE_TABLETOP_NO_PLANE_FIRST, OPE_TABLETOP_NO_PLANE_SECOND,
         OPE_PLANE_MAX_ITERATIONS);
  return 0;
}
"""


def test_plane_layouts_match_the_c_compiler(ope, tmp_path):
    c = tmp_path / "probe.c"
    c.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.check_call(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)], text=True).splitlines()
    want = {ln.split(" ", 1)[0]: ln.split(" ", 1)[1] for ln in lines}
    structs = {"p": ope.PlaneParams, "s": ope.PlaneStats, "t": ope.TabletopResult}
    got = {"sizeof_" + t: str(ctypes.sizeof(S)) for t, S in structs.items()}
    for t, S in structs.items():
        for name, _ in S._fields_:
            got[t + "." + name] = str(getattr(S, name).offset)
    got["abi"] = "5"   # the change only adds to the ABI
    got["status"] = "%d %d %d" % (ope.TABLETOP_OK, ope.TABLETOP_NO_PLANE_FIRST, ope.TABLETOP_NO_PLANE_SECOND)
    got["maxit"] = "1023"
    assert got == want


def test_plane_defaults_are_the_reference_literals(ope):
    p = ope.default_plane_params()
    assert p.distance_threshold == 0.01      # setDistanceThreshold (0.01) (objectsegmentationplane.cpp:43)
    assert p.max_iterations == 50            # SACSegmentation: max_iterations_ (50)
    assert p.probability == 0.99             # SACSegmentation: probability_ (0.99)
    assert p.optimize_coefficients == 1      # setOptimizeCoefficients (true) (:39)
    assert p.seed == 12345                   # SampleConsensusModel: rng_alg_.seed (12345u) when random is false
    assert ope.default_plane_params(seed=7).seed == 7
