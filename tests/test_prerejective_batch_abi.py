"""CPU-side checks of the batched prerejective entries: declared, exported and bound; the ctypes structs lay out exactly as the C
compiler lays out ope_prerejective_batch_result / _stats; the structs the new entries take and fill did not change size."""
import ctypes
import os
import re
import subprocess

import pytest

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


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "ope.h"
#define O(t, tag, m) printf("%s.%s %zu\n", tag, #m, offsetof(t, m))
int main(void) {
  printf("sizeof_r %zu\nsizeof_s %zu\n", sizeof(ope_prerejective_batch_result), sizeof(ope_prerejective_batch_stats));
  printf("sizeof_params %zu\nsizeof_coarse %zu\nsizeof_final %zu\n", sizeof(ope_prerejective_params), sizeof(ope_coarse_params),
         sizeof(ope_final_batch_result));
  O(ope_prerejective_batch_result, "r", T); O(ope_prerejective_batch_result, "r", error); O(ope_prerejective_batch_result, "r", best_iteration);
  O(ope_prerejective_batch_result, "r", inliers); O(ope_prerejective_batch_result, "r", converged); O(ope_prerejective_batch_result, "r", survivors);
  O(ope_prerejective_batch_result, "r", n_src_keys); O(ope_prerejective_batch_result, "r", n_tgt_keys); O(ope_prerejective_batch_result, "r", status);
  O(ope_prerejective_batch_result, "r", seed);
  O(ope_prerejective_batch_stats, "s", clusters); O(ope_prerejective_batch_stats, "s", active); O(ope_prerejective_batch_stats, "s", iterations);
  O(ope_prerejective_batch_stats, "s", survivors); O(ope_prerejective_batch_stats, "s", launches); O(ope_prerejective_batch_stats, "s", host_syncs);
  O(ope_prerejective_batch_stats, "s", nr_samples);
  printf("enum %d %d %d %d\n", OPE_PREREJ_OK, OPE_PREREJ_EMPTY_TARGET, OPE_PREREJ_FEW_TARGET_FEATURES, OPE_PREREJ_NAN_FEATURES);
  printf("abi %d\n", OPE_ABI_VERSION);
  return 0;
}
"""


def test_batch_layouts_match_the_c_compiler(ope, tmp_path):
    c = tmp_path / "probe.c"
    c.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.check_call(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)], text=True).splitlines()
    want = {ln.split(" ", 1)[0]: ln.split(" ", 1)[1] for ln in lines}
    structs = {"r": ope.PrerejectiveBatchResult, "s": ope.PrerejectiveBatchStats}
    got = {"sizeof_" + t: str(ctypes.sizeof(S)) for t, S in structs.items()}
    for t, S in structs.items():
        for name, _ in S._fields_:
            got[t + "." + name] = str(getattr(S, name).offset)
    got["sizeof_params"] = str(ctypes.sizeof(ope.PrerejectiveParams))
    got["sizeof_coarse"] = str(ctypes.sizeof(ope.CoarseParams))
    got["sizeof_final"] = str(ctypes.sizeof(ope.FinalBatchResult))
    got["enum"] = " ".join(str(v) for v in (ope.PREREJ_OK, ope.PREREJ_EMPTY_TARGET, ope.PREREJ_FEW_TARGET_FEATURES, ope.PREREJ_NAN_FEATURES))
    got["abi"] = "5"   # the change only adds to the ABI
    assert got == want
    # the layouts, pinned; the three existing structs as they were before the batch
    assert (got["sizeof_r"], got["sizeof_s"]) == ("112", "56")
    assert [got["r." + n] for n, _ in ope.PrerejectiveBatchResult._fields_] == ["0", "64", "72", "76", "80", "84", "88", "92", "96", "104"]
    assert [n for n, _ in ope.PrerejectiveBatchStats._fields_] == ["clusters", "active", "iterations", "survivors", "launches", "host_syncs",
                                                                   "nr_samples"]
    assert (got["sizeof_params"], got["sizeof_coarse"], got["sizeof_final"]) == ("40", "64", "232")
