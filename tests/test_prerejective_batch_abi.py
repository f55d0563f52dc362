"""CPU-side checks of the batched prerejective entries: declared, exported and bound; the ctypes structs lay out exactly as the C
compiler lays out ope_prerejective_batch_result / _stats; the structs the new entries take and fill did not change size."""
import ctypes
import os
import re

import pytest

from abi_probe import c_layout, ctypes_layout
from conftest import ROOT, load_pkg

HEADER = os.path.join(ROOT, "include", "ope.h")
ENTRIES = ("ope_prerejective_pose_batch", "ope_prerejective_batch_last_stats", "ope_prerejective_batch_hypotheses",
           "ope_final_pose_batch_prerejective")


@pytest.fixture(scope="module")
def ope():
    pkg = load_pkg()
    pkg.build_library()
    return pkg


@pytest.mark.parametrize("name", ENTRIES)
def test_batch_entry_is_declared_exported_and_bound(ope, name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+" + name + r"\s*\(", src)
    assert hasattr(ctypes.CDLL(ope.LIB_PATH), name)
    assert name in {n for n, _, _ in ope.ABI}
    fn = getattr(ope.lib(), name)
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == {"ope_prerejective_pose_batch": 9, "ope_prerejective_batch_last_stats": 2,
                                                                "ope_prerejective_batch_hypotheses": 10,
                                                                "ope_final_pose_batch_prerejective": 9}[name]
    for method in ("prerejective_pose_batch", "prerejective_batch_stats", "prerejective_batch_hypotheses", "final_pose_batch_prerejective"):
        assert callable(getattr(ope.Context, method))


def test_batch_layouts_match_the_c_compiler(ope):
    R, S = "ope_prerejective_batch_result", "ope_prerejective_batch_stats"
    structs = {ope.PrerejectiveBatchResult: R, ope.PrerejectiveBatchStats: S, ope.PrerejectiveParams: "ope_prerejective_params",
               ope.CoarseParams: "ope_coarse_params", ope.FinalBatchResult: "ope_final_batch_result"}
    got = {k: str(v) for k, v in ctypes_layout(structs).items()}
    got["status.ok"], got["status.empty"], got["status.few"], got["status.nan"] = (
        str(v) for v in (ope.PREREJ_OK, ope.PREREJ_EMPTY_TARGET, ope.PREREJ_FEW_TARGET_FEATURES, ope.PREREJ_NAN_FEATURES))
    got["abi"] = "5"   # the change only adds to the ABI
    want = c_layout(structs, extra={"status.ok": "OPE_PREREJ_OK", "status.empty": "OPE_PREREJ_EMPTY_TARGET",
                                    "status.few": "OPE_PREREJ_FEW_TARGET_FEATURES", "status.nan": "OPE_PREREJ_NAN_FEATURES",
                                    "abi": "OPE_ABI_VERSION"})
    assert got == {k: str(v) for k, v in want.items()}
    # the layouts, pinned; the three existing structs as they were before the batch
    assert (got[R, "sizeof"], got[S, "sizeof"]) == ("112", "56")
    assert [got[R, n] for n, _ in ope.PrerejectiveBatchResult._fields_] == ["0", "64", "72", "76", "80", "84", "88", "92", "96", "104"]
    assert [n for n, _ in ope.PrerejectiveBatchStats._fields_] == ["clusters", "active", "iterations", "survivors", "launches", "host_syncs",
                                                                   "nr_samples"]
    assert (got["ope_prerejective_params", "sizeof"], got["ope_coarse_params", "sizeof"], got["ope_final_batch_result", "sizeof"]) == (
        "40", "64", "232")
