"""CPU-side checks of region growing (ope_region_grow, ope_region_grow_cloud): declared, exported and bound; the ctypes structs lay
out exactly as the C compiler lays out ope_region_params / ope_region_stats; the defaults are the reference's literals
(segmentationregiongrow.cpp:25-36)."""
import ctypes
import math
import os
import re
import subprocess

import pytest

from conftest import ROOT, load_pkg

HEADER = os.path.join(ROOT, "include", "ope.h")
ENTRIES = ("ope_region_default_params", "ope_region_grow", "ope_region_grow_cloud", "ope_region_last_stats")


@pytest.fixture(scope="module")
def ope():
    pkg = load_pkg()
    pkg.build_library()
    return pkg


@pytest.mark.parametrize("name", ENTRIES)
def test_region_entry_is_declared_exported_and_bound(ope, name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\b(int|void)\s+" + name + r"\s*\(", src)
    assert hasattr(ctypes.CDLL(ope.LIB_PATH), name)
    assert name in {n for n, _, _ in ope.ABI}


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "ope.h"
#define O(t, tag, m) printf("%s.%s %zu\n", tag, #m, offsetof(t, m))
int main(void) {
  printf("sizeof_p %zu\nsizeof_s %zu\n", sizeof(ope_region_params), sizeof(ope_region_stats));
  O(ope_region_params, "p", number_of_neighbours); O(ope_region_params, "p", normals_k); O(ope_region_params, "p", smoothness_threshold);
  O(ope_region_params, "p", curvature_threshold); O(ope_region_params, "p", min_size); O(ope_region_params, "p", max_size);
  O(ope_region_stats, "s", launches); O(ope_region_stats, "s", host_syncs); O(ope_region_stats, "s", sweeps);
  O(ope_region_stats, "s", one_way_edges); O(ope_region_stats, "s", regions_before_size_filter); O(ope_region_stats, "s", refused_curvature);
  return 0;
}
"""


def test_region_layouts_match_the_c_compiler(ope, tmp_path):
    c = tmp_path / "probe.c"
    c.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.check_call(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    want = dict(line.rsplit(" ", 1) for line in subprocess.check_output([str(exe)], text=True).splitlines())
    want = {k: int(v) for k, v in want.items()}
    structs = {"p": ope.RegionParams, "s": ope.RegionStats}
    got = {"sizeof_" + t: ctypes.sizeof(S) for t, S in structs.items()}
    for t, S in structs.items():
        for name, _ in S._fields_:
            got[t + "." + name] = getattr(S, name).offset
    assert got == want


def test_region_binding_has_the_header_s_argument_counts(ope):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    table = {n: a for n, _, a in ope.ABI}
    for name in ENTRIES:
        args = re.search(r"\b" + name + r"\s*\(([^)]*)\)", src).group(1)
        assert len(args.split(",")) == len(table[name]), name


def test_region_defaults_are_the_reference_literals(ope):
    p = ope.default_region_params()
    assert p.number_of_neighbours == 15                       # setNumberOfNeighbours (15) (segmentationregiongrow.cpp:31)
    assert p.normals_k == 30                                  # setKSearch (30) (:25)
    assert p.smoothness_threshold == 10.0 / 180.0 * math.pi   # setSmoothnessThreshold (10.0 / 180.0 * M_PI) (:35)
    assert p.curvature_threshold == 1.0                       # setCurvatureThreshold (1.0) (:36)
    assert (p.min_size, p.max_size) == (500, 1000000)         # setMinClusterSize (500), setMaxClusterSize (1000000) (:28-29)
    assert ope.default_region_params(min_size=1).min_size == 1
