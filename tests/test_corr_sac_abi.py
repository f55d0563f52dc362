"""CPU-side checks of the correspondence-rejection entries: declared, exported and bound; the ctypes structs lay out exactly as the C
compiler lays out ope_corr_sac_params / _result / _stats; the defaults are PCL's own."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT, load_pkg

HEADER = os.path.join(ROOT, "include", "ope.h")
ENTRIES = ("ope_feature_correspondences", "ope_corr_sac_default_params", "ope_corr_sac", "ope_corr_sac_last_stats",
           "ope_corr_sac_last_hypotheses")


@pytest.fixture(scope="module")
def ope():
    pkg = load_pkg()
    pkg.build_library()
    return pkg


@pytest.mark.parametrize("name", ENTRIES)
def test_corr_sac_entry_is_declared_exported_and_bound(ope, name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\b(int|void)\s+" + name + r"\s*\(", src)
    assert hasattr(ctypes.CDLL(ope.LIB_PATH), name)
    assert name in {n for n, _, _ in ope.ABI}
    for method in ("feature_correspondences", "corr_sac", "corr_sac_stats", "corr_sac_hypotheses", "coarse_pose_correspondences"):
        assert callable(getattr(ope.Context, method))
    assert callable(ope.default_corr_sac_params)


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "ope.h"
#define O(t, tag, m) printf("%s.%s %zu\n", tag, #m, offsetof(t, m))
int main(void) {
  printf("sizeof_p %zu\nsizeof_r %zu\nsizeof_s %zu\n", sizeof(ope_corr_sac_params), sizeof(ope_corr_sac_result), sizeof(ope_corr_sac_stats));
  O(ope_corr_sac_params, "p", inlier_threshold); O(ope_corr_sac_params, "p", max_iterations); O(ope_corr_sac_params, "p", probability);
  O(ope_corr_sac_params, "p", seed);
  O(ope_corr_sac_result, "r", T_best); O(ope_corr_sac_result, "r", T_svd); O(ope_corr_sac_result, "r", inliers);
  O(ope_corr_sac_result, "r", best); O(ope_corr_sac_result, "r", iterations); O(ope_corr_sac_result, "r", found);
  O(ope_corr_sac_stats, "s", hypotheses); O(ope_corr_sac_stats, "s", iterations); O(ope_corr_sac_stats, "s", launches);
  O(ope_corr_sac_stats, "s", host_syncs); O(ope_corr_sac_stats, "s", sample_dist_thresh);
  printf("abi %d\n", OPE_ABI_VERSION);
  return 0;
}
"""


def test_corr_sac_layouts_match_the_c_compiler(ope, tmp_path):
    c = tmp_path / "probe.c"
    c.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.check_call(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)], text=True).splitlines()
    want = {ln.split(" ", 1)[0]: ln.split(" ", 1)[1] for ln in lines}
    structs = {"p": ope.CorrSacParams, "r": ope.CorrSacResult, "s": ope.CorrSacStats}
    got = {"sizeof_" + t: str(ctypes.sizeof(S)) for t, S in structs.items()}
    for t, S in structs.items():
        for name, _ in S._fields_:
            got[t + "." + name] = str(getattr(S, name).offset)
    got["abi"] = "5"   # the change only adds to the ABI
    assert got == want
    # the layout itself, pinned
    assert (got["sizeof_p"], got["sizeof_r"], got["sizeof_s"]) == ("32", "144", "40")
    assert [got["p." + n] for n, _ in ope.CorrSacParams._fields_] == ["0", "8", "16", "24"]
    assert [got["r." + n] for n, _ in ope.CorrSacResult._fields_] == ["0", "64", "128", "132", "136", "140"]
    assert [n for n, _ in ope.CorrSacStats._fields_] == ["hypotheses", "iterations", "launches", "host_syncs", "sample_dist_thresh"]


def test_corr_sac_defaults_are_pcls(ope):
    p = ope.default_corr_sac_params()
    assert p.inlier_threshold == 0.05      # CorrespondenceRejectorSampleConsensus::inlier_threshold_
    assert p.max_iterations == 1000        # ::max_iterations_
    assert p.probability == 0.99           # SampleConsensus::probability_
    assert p.seed == 12345                 # SampleConsensusModel's engine without a random seed
    q = ope.default_corr_sac_params(inlier_threshold=0.08, max_iterations=10000)   # BuildModel/src/poseestimator.cpp:55-56
    assert q.inlier_threshold == 0.08 and q.max_iterations == 10000
    with pytest.raises(AttributeError):
        ope.default_corr_sac_params(no_such_field=1)
