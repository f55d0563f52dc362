"""CPU-side checks of the prerejective alignment entries: declared, exported and bound; the ctypes structs lay out exactly as the C
compiler lays out ope_prerejective_params / _result / _stats; the defaults are the values of the reference's commented block
(BuildModel/src/poseestimator.cpp:97-102)."""
import ctypes
import os
import re

import pytest

from abi_probe import c_layout, ctypes_layout
from conftest import ROOT, load_pkg

HEADER = os.path.join(ROOT, "include", "ope.h")
ENTRIES = ("ope_prerejective_default_params", "ope_prerejective", "ope_prerejective_last_stats", "ope_prerejective_last_hypotheses")


@pytest.fixture(scope="module")
def ope():
    pkg = load_pkg()
    pkg.build_library()
    return pkg


@pytest.mark.parametrize("name", ENTRIES)
def test_prerejective_entry_is_declared_exported_and_bound(ope, name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\b(int|void)\s+" + name + r"\s*\(", src)
    assert hasattr(ctypes.CDLL(ope.LIB_PATH), name)
    assert name in {n for n, _, _ in ope.ABI}
    for method in ("prerejective", "prerejective_stats", "prerejective_hypotheses"):
        assert callable(getattr(ope.Context, method))


def test_prerejective_layouts_match_the_c_compiler(ope):
    P, R, S = "ope_prerejective_params", "ope_prerejective_result", "ope_prerejective_stats"
    structs = {ope.PrerejectiveParams: P, ope.PrerejectiveResult: R, ope.PrerejectiveStats: S}
    got = {k: str(v) for k, v in ctypes_layout(structs).items()}
    got["abi"] = "5"   # the change only adds to the ABI
    assert got == {k: str(v) for k, v in c_layout(structs, extra={"abi": "OPE_ABI_VERSION"}).items()}
    # the layout itself, pinned
    assert (got[P, "sizeof"], got[R, "sizeof"], got[S, "sizeof"]) == ("40", "88", "40")
    assert [got[P, n] for n, _ in ope.PrerejectiveParams._fields_] == ["0", "4", "8", "12", "16", "24", "32"]
    assert [got[R, n] for n, _ in ope.PrerejectiveResult._fields_] == ["0", "64", "72", "76", "80"]
    assert [n for n, _ in ope.PrerejectiveStats._fields_] == ["iterations", "survivors", "launches", "host_syncs", "nr_samples"]


def test_prerejective_defaults_are_the_reference_literals(ope):
    p = ope.default_prerejective_params()
    assert p.max_iterations == 50000                        # setMaximumIterations (50000) (:97)
    assert p.nr_samples == 3                                # setNumberOfSamples (3) (:98)
    assert p.k_correspondences == 5                         # setCorrespondenceRandomness (5) (:99)
    assert p.similarity_threshold == pytest.approx(0.8)     # setSimilarityThreshold (0.8f) (:100)
    assert ctypes.c_float(p.similarity_threshold).value == ctypes.c_float(0.8).value
    assert p.max_corr_dist == 0.15                          # setMaxCorrespondenceDistance (:101)
    assert ctypes.c_float(p.inlier_fraction).value == 0.25  # setInlierFraction (0.25f) (:102)
    assert p.seed == 1
    assert ope.default_prerejective_params(seed=7, max_iterations=10).seed == 7
    with pytest.raises(AttributeError):
        ope.default_prerejective_params(no_such_field=1)
