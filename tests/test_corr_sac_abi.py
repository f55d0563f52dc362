"""CPU-side checks of the correspondence-rejection entries: declared, exported and bound; the ctypes structs lay out exactly as the C
compiler lays out ope_corr_sac_params / _result / _stats; the defaults are PCL's own."""
import ctypes
import os
import re

import pytest

from abi_probe import c_layout, ctypes_layout
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


def test_corr_sac_layouts_match_the_c_compiler(ope):
    P, R, S = "ope_corr_sac_params", "ope_corr_sac_result", "ope_corr_sac_stats"
    structs = {ope.CorrSacParams: P, ope.CorrSacResult: R, ope.CorrSacStats: S}
    got = {k: str(v) for k, v in ctypes_layout(structs).items()}
    got["abi"] = "5"   # the change only adds to the ABI
    assert got == {k: str(v) for k, v in c_layout(structs, extra={"abi": "OPE_ABI_VERSION"}).items()}
    # the layout itself, pinned
    assert (got[P, "sizeof"], got[R, "sizeof"], got[S, "sizeof"]) == ("32", "144", "40")
    assert [got[P, n] for n, _ in ope.CorrSacParams._fields_] == ["0", "8", "16", "24"]
    assert [got[R, n] for n, _ in ope.CorrSacResult._fields_] == ["0", "64", "128", "132", "136", "140"]
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
