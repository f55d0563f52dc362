"""CPU-side checks of the batched final pose (ope_final_pose_batch): declared, exported and bound; the ctypes structs of its
parameters and per-cluster result lay out exactly as the C compiler lays out ope_final_params / ope_final_batch_result; the
defaults are the reference's values."""
import ctypes
import os
import re

import pytest

from abi_probe import c_layout, ctypes_layout
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


def test_final_layouts_match_the_c_compiler(ope):
    structs = {ope.FinalParams: "ope_final_params", ope.FinalBatchResult: "ope_final_batch_result"}
    got = ctypes_layout(structs)
    got["status.ok"], got["status.empty"] = ope.FINAL_OK, ope.FINAL_EMPTY_TARGET
    got["status.few_features"], got["status.few_fine"] = ope.FINAL_FEW_TARGET_FEATURES, ope.FINAL_FEW_FINE_POINTS
    got["abi"] = 5   # the change only adds to the ABI
    assert got == c_layout(structs, extra={"status.ok": "OPE_FINAL_OK", "status.empty": "OPE_FINAL_EMPTY_TARGET",
                                           "status.few_features": "OPE_FINAL_FEW_TARGET_FEATURES",
                                           "status.few_fine": "OPE_FINAL_FEW_FINE_POINTS", "abi": "OPE_ABI_VERSION"})


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
