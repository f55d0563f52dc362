"""CPU-side checks of the batched coarse stage (ope_coarse_pose_batch): declared, exported and bound; the ctypes structs of its
parameters and per-cluster result lay out exactly as the C compiler lays out ope_coarse_params / ope_coarse_batch_result; the
defaults are the reference's values."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT, load_pkg

HEADER = os.path.join(ROOT, "include", "ope.h")
ENTRIES = ("ope_coarse_pose_batch", "ope_coarse_batch_features", "ope_coarse_default_params")


@pytest.fixture(scope="module")
def ope():
    pkg = load_pkg()
    pkg.build_library()
    return pkg


@pytest.mark.parametrize("name", ENTRIES)
def test_coarse_entry_is_declared_exported_and_bound(ope, name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\b(int|void)\s+" + name + r"\s*\(", src)
    assert hasattr(ctypes.CDLL(ope.LIB_PATH), name)
    assert name in {n for n, _, _ in ope.ABI}


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "ope.h"
#define P(m) printf("p.%s %zu\n", #m, offsetof(ope_coarse_params, m))
#define S(m) printf("p.sacia.%s %zu\n", #m, offsetof(ope_coarse_params, sacia) + offsetof(ope_sacia_params, m))
#define R(m) printf("r.%s %zu\n", #m, offsetof(ope_coarse_batch_result, m))
int main(void) {
  printf("sizeof_p %zu\nsizeof_r %zu\n", sizeof(ope_coarse_params), sizeof(ope_coarse_batch_result));
  P(key_leaf); P(normals_k); P(viewpoint); P(fpfh_radius); P(sacia);
  S(max_iterations); S(nr_samples); S(k_correspondences); S(max_corr_dist); S(min_sample_dist); S(seed);
  R(T); R(best_error); R(best_iteration); R(n_src_keys); R(n_tgt_keys); R(status);
  printf("limits.points %d\nlimits.keys %d\n", OPE_COARSE_MAX_POINTS, OPE_COARSE_MAX_KEYS);
  printf("status.ok %d\nstatus.empty %d\nstatus.few %d\n", OPE_COARSE_OK, OPE_COARSE_EMPTY_TARGET, OPE_COARSE_FEW_TARGET_FEATURES);
  return 0;
}
"""


def test_coarse_layouts_match_the_c_compiler(ope, tmp_path):
    c = tmp_path / "probe.c"
    c.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.check_call(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    want = dict(line.rsplit(" ", 1) for line in subprocess.check_output([str(exe)], text=True).splitlines())
    want = {k: int(v) for k, v in want.items()}
    P, S, R = ope.CoarseParams, ope.SaciaParams, ope.CoarseBatchResult
    got = {"sizeof_p": ctypes.sizeof(P), "sizeof_r": ctypes.sizeof(R)}
    for name, _ in P._fields_:
        got["p." + name] = getattr(P, name).offset
    for name, _ in S._fields_:
        got["p.sacia." + name] = P.sacia.offset + getattr(S, name).offset
    for name, _ in R._fields_:
        got["r." + name] = getattr(R, name).offset
    got["limits.points"], got["limits.keys"] = ope.COARSE_MAX_POINTS, ope.COARSE_MAX_KEYS
    got["status.ok"], got["status.empty"], got["status.few"] = ope.COARSE_OK, ope.COARSE_EMPTY_TARGET, ope.COARSE_FEW_TARGET_FEATURES
    assert got == want


def test_coarse_defaults_are_the_reference_values(ope):
    p = ope.default_coarse_params()
    assert p.key_leaf == ctypes.c_float(0.01).value            # UniformSampling radius (poseestimator.cpp:116)
    assert p.normals_k == 30                                    # (:153)
    assert list(p.viewpoint) == [0.0, 0.0, 0.0]                 # NormalEstimation's default viewpoint
    assert p.fpfh_radius == ctypes.c_float(0.03).value          # (:122)
    s = p.sacia
    assert (s.max_iterations, s.nr_samples, s.k_correspondences) == (400, 5, 5)
    assert s.max_corr_dist == 0.05 and s.min_sample_dist == ctypes.c_float(0.01).value and s.seed == 1
    q = ope.default_coarse_params(normals_k=12, viewpoint=(1, 2, 3))
    assert q.normals_k == 12 and list(q.viewpoint) == [1.0, 2.0, 3.0]
