"""CPU-side checks of the batched final pose (ope_final_pose_batch): declared, exported and bound; the ctypes structs of its
parameters and per-cluster result lay out exactly as the C compiler lays out ope_final_params / ope_final_batch_result; the
defaults are the reference's values."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT, load_pkg

HEADER = os.path.join(ROOT, "include", "ope.h")
ENTRIES = ("ope_final_pose_batch", "ope_final_batch_inputs", "ope_final_default_params")


@pytest.fixture(scope="module")
def ope():
    pkg = load_pkg()
    pkg.build_library()
    return pkg


@pytest.mark.parametrize("name", ENTRIES)
def test_final_entry_is_declared_exported_and_bound(ope, name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\b(int|void)\s+" + name + r"\s*\(", src)
    assert hasattr(ctypes.CDLL(ope.LIB_PATH), name)
    assert name in {n for n, _, _ in ope.ABI}


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "ope.h"
#define P(m) printf("p.%s %zu\n", #m, offsetof(ope_final_params, m))
#define R(m) printf("r.%s %zu\n", #m, offsetof(ope_final_batch_result, m))
int main(void) {
  printf("sizeof_p %zu\nsizeof_r %zu\n", sizeof(ope_final_params), sizeof(ope_final_batch_result));
  P(coarse); P(fine_leaf); P(fine_normals_k); P(min_fine_points); P(icp); P(fitness_max_range); P(accept_fitness); P(accept_strength);
  R(coarse); R(seed); R(fine); R(n_fine_src); R(n_fine_tgt); R(status); R(accepted);
  printf("status.ok %d\nstatus.empty %d\nstatus.few_features %d\nstatus.few_fine %d\n", OPE_FINAL_OK, OPE_FINAL_EMPTY_TARGET,
         OPE_FINAL_FEW_TARGET_FEATURES, OPE_FINAL_FEW_FINE_POINTS);
  printf("abi %d\n", OPE_ABI_VERSION);
  return 0;
}
"""


def test_final_layouts_match_the_c_compiler(ope, tmp_path):
    c = tmp_path / "probe.c"
    c.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.check_call(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    want = dict(line.rsplit(" ", 1) for line in subprocess.check_output([str(exe)], text=True).splitlines())
    want = {k: int(v) for k, v in want.items()}
    P, R = ope.FinalParams, ope.FinalBatchResult
    got = {"sizeof_p": ctypes.sizeof(P), "sizeof_r": ctypes.sizeof(R)}
    for name, _ in P._fields_:
        got["p." + name] = getattr(P, name).offset
    for name, _ in R._fields_:
        got["r." + name] = getattr(R, name).offset
    got["status.ok"], got["status.empty"] = ope.FINAL_OK, ope.FINAL_EMPTY_TARGET
    got["status.few_features"], got["status.few_fine"] = ope.FINAL_FEW_TARGET_FEATURES, ope.FINAL_FEW_FINE_POINTS
    got["abi"] = 5   # the change only adds to the ABI
    assert got == want


def test_final_defaults_are_the_reference_values(ope):
    p = ope.default_final_params()
    c = ope.default_coarse_params()
    assert bytes(p.coarse) == bytes(c)                               # ope_coarse_default_params
    assert p.fine_leaf == ctypes.c_float(0.008).value               # withNormals' sub-sampling (poseestimator.cpp:196-216)
    assert p.fine_normals_k == 30
    assert p.min_fine_points == 100                                 # (:218-223)
    i = p.icp
    assert (i.max_iterations, i.transformation_epsilon, i.euclidean_fitness_epsilon) == (100, 1e-8, 1e-8)   # (:322-328)
    assert (i.corr_mode, i.k_normal_shooting) == (ope.CORR_NORMAL_SHOOTING, 20)                              # (:246)
    assert (i.use_surface_normal_rej, i.surface_normal_thr) == (1, 0.7)                                      # (:272)
    assert i.use_self_occluded_rej == 0 and i.use_reciprocal == 0 and i.estimator == ope.EST_SVD
    assert p.fitness_max_range == float.fromhex("0x1.fffffffffffffp+1023")   # getFitnessScore's default, DBL_MAX
    assert (p.accept_fitness, p.accept_strength) == (1e-4, 0.4)              # rosinterface.cpp:256
