"""CPU-side checks of the batched coarse stage (ope_coarse_pose_batch): declared, exported and bound; the ctypes structs of its
parameters and per-cluster result lay out exactly as the C compiler lays out ope_coarse_params / ope_coarse_batch_result; the
defaults are the reference's values."""
import ctypes
import os
import re

import pytest

from abi_probe import c_layout, ctypes_layout
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


def test_coarse_layouts_match_the_c_compiler(ope):
    structs = {ope.CoarseParams: "ope_coarse_params", ope.SaciaParams: "ope_sacia_params", ope.CoarseBatchResult: "ope_coarse_batch_result"}
    got = ctypes_layout(structs)
    got["limits.points"], got["limits.keys"] = ope.COARSE_MAX_POINTS, ope.COARSE_MAX_KEYS
    got["status.ok"], got["status.empty"], got["status.few"] = ope.COARSE_OK, ope.COARSE_EMPTY_TARGET, ope.COARSE_FEW_TARGET_FEATURES
    assert got == c_layout(structs, extra={"limits.points": "OPE_COARSE_MAX_POINTS", "limits.keys": "OPE_COARSE_MAX_KEYS",
                                           "status.ok": "OPE_COARSE_OK", "status.empty": "OPE_COARSE_EMPTY_TARGET",
                                           "status.few": "OPE_COARSE_FEW_TARGET_FEATURES"})


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
