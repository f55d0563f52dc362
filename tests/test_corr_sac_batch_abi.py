"""CPU-side checks of the batched correspondence aligner's entries: declared, exported and bound; the ctypes structs lay out exactly
as the C compiler lays out ope_corr_sac_batch_result / _stats; the status constants."""
import ctypes
import os
import re

import pytest

from abi_probe import c_layout, ctypes_layout
from conftest import ROOT, load_pkg

HEADER = os.path.join(ROOT, "include", "ope.h")
ENTRIES = ("ope_corr_sac_pose_batch", "ope_corr_sac_batch_last_stats", "ope_corr_sac_batch_matches", "ope_corr_sac_batch_inliers",
           "ope_corr_sac_batch_hypotheses", "ope_final_pose_batch_correspondences")
METHODS = ("corr_sac_pose_batch", "corr_sac_batch_stats", "corr_sac_batch_matches", "corr_sac_batch_inliers", "corr_sac_batch_hypotheses",
           "final_pose_batch_correspondences")


@pytest.fixture(scope="module")
def ope():
    pkg = load_pkg()
    pkg.build_library()
    return pkg


@pytest.mark.parametrize("name", ENTRIES)
def test_corr_sac_batch_entry_is_declared_exported_and_bound(ope, name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+" + name + r"\s*\(", src)
    assert hasattr(ctypes.CDLL(ope.LIB_PATH), name)
    assert name in {n for n, _, _ in ope.ABI}
    for method in METHODS:
        assert callable(getattr(ope.Context, method))


def test_corr_sac_batch_layouts_match_the_c_compiler(ope):
    R, S = "ope_corr_sac_batch_result", "ope_corr_sac_batch_stats"
    structs = {ope.CorrSacBatchResult: R, ope.CorrSacBatchStats: S}
    got = {k: str(v) for k, v in ctypes_layout(structs).items()}
    got["status.ok"], got["status.empty"], got["status.few"] = (str(v) for v in (ope.CORRSAC_OK, ope.CORRSAC_EMPTY_TARGET,
                                                                                 ope.CORRSAC_FEW_TARGET_FEATURES))
    got["abi"] = "5"   # the change only adds to the ABI
    want = c_layout(structs, extra={"status.ok": "OPE_CORRSAC_OK", "status.empty": "OPE_CORRSAC_EMPTY_TARGET",
                                    "status.few": "OPE_CORRSAC_FEW_TARGET_FEATURES", "abi": "OPE_ABI_VERSION"})
    assert got == {k: str(v) for k, v in want.items()}
    assert (got[R, "sizeof"], got[S, "sizeof"]) == ("176", "48")
    assert [got[R, n] for n, _ in ope.CorrSacBatchResult._fields_] == ["0", "64", "128", "136", "144", "148", "152", "156", "160", "164",
                                                                       "168", "172"]
    assert [n for n, _ in ope.CorrSacBatchStats._fields_] == ["clusters", "active", "hypotheses", "draw_lists", "launches", "host_syncs"]


def test_corr_sac_batch_status_constants(ope):
    assert (ope.CORRSAC_OK, ope.CORRSAC_EMPTY_TARGET, ope.CORRSAC_FEW_TARGET_FEATURES) == (0, 1, 2)
