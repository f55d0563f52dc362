"""CPU-side checks of the batched correspondence aligner's entries: declared, exported and bound; the ctypes structs lay out exactly
as the C compiler lays out ope_corr_sac_batch_result / _stats; the status constants."""
import ctypes
import os
import re
import subprocess

import pytest

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


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "ope.h"
#define O(t, tag, m) printf("%s.%s %zu\n", tag, #m, offsetof(t, m))
int main(void) {
  printf("sizeof_r %zu\nsizeof_s %zu\n", sizeof(ope_corr_sac_batch_result), sizeof(ope_corr_sac_batch_stats));
  O(ope_corr_sac_batch_result, "r", T_svd); O(ope_corr_sac_batch_result, "r", T_best); O(ope_corr_sac_batch_result, "r", sample_dist_thresh);
  O(ope_corr_sac_batch_result, "r", seed); O(ope_corr_sac_batch_result, "r", matches); O(ope_corr_sac_batch_result, "r", inliers);
  O(ope_corr_sac_batch_result, "r", best); O(ope_corr_sac_batch_result, "r", iterations); O(ope_corr_sac_batch_result, "r", found);
  O(ope_corr_sac_batch_result, "r", n_src_keys); O(ope_corr_sac_batch_result, "r", n_tgt_keys); O(ope_corr_sac_batch_result, "r", status);
  O(ope_corr_sac_batch_stats, "s", clusters); O(ope_corr_sac_batch_stats, "s", active); O(ope_corr_sac_batch_stats, "s", hypotheses);
  O(ope_corr_sac_batch_stats, "s", draw_lists); O(ope_corr_sac_batch_stats, "s", launches); O(ope_corr_sac_batch_stats, "s", host_syncs);
  printf("status %d %d %d\n", OPE_CORRSAC_OK, OPE_CORRSAC_EMPTY_TARGET, OPE_CORRSAC_FEW_TARGET_FEATURES);
  printf("abi %d\n", OPE_ABI_VERSION);
  return 0;
}
"""


def test_corr_sac_batch_layouts_match_the_c_compiler(ope, tmp_path):
    c = tmp_path / "probe.c"
    c.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.check_call(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)], text=True).splitlines()
    want = {ln.split(" ", 1)[0]: ln.split(" ", 1)[1] for ln in lines}
    structs = {"r": ope.CorrSacBatchResult, "s": ope.CorrSacBatchStats}
    got = {"sizeof_" + t: str(ctypes.sizeof(S)) for t, S in structs.items()}
    for t, S in structs.items():
        for name, _ in S._fields_:
            got[t + "." + name] = str(getattr(S, name).offset)
    got["status"] = f"{ope.CORRSAC_OK} {ope.CORRSAC_EMPTY_TARGET} {ope.CORRSAC_FEW_TARGET_FEATURES}"
    got["abi"] = "5"   # the change only adds to the ABI
    assert got == want
    assert (got["sizeof_r"], got["sizeof_s"]) == ("176", "48")
    assert [got["r." + n] for n, _ in ope.CorrSacBatchResult._fields_] == ["0", "64", "128", "136", "144", "148", "152", "156", "160", "164",
                                                                          "168", "172"]
    assert [n for n, _ in ope.CorrSacBatchStats._fields_] == ["clusters", "active", "hypotheses", "draw_lists", "launches", "host_syncs"]


def test_corr_sac_batch_status_constants(ope):
    assert (ope.CORRSAC_OK, ope.CORRSAC_EMPTY_TARGET, ope.CORRSAC_FEW_TARGET_FEATURES) == (0, 1, 2)
