"""CPU-side checks of tracking (ope_track_gate, ope_track_pose): declared, exported and bound; the ctypes structs lay out
exactly as the C compiler lays out ope_track_params / ope_track_centroid / ope_track_gate_result / ope_track_result; the
defaults are the reference's literals (rosinterface.cpp:279,304, poseestimator.cpp:399)."""
import ctypes
import os
import re

import pytest

from abi_probe import c_layout, ctypes_layout
from conftest import ROOT, load_pkg

HEADER = os.path.join(ROOT, "include", "ope.h")
ENTRIES = ("ope_track_default_params", "ope_track_gate", "ope_track_pose")


@pytest.fixture(scope="module")
def ope():
    pkg = load_pkg()
    pkg.build_library()
    return pkg


@pytest.mark.parametrize("name", ENTRIES)
def test_track_entry_is_declared_exported_and_bound(ope, name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\b(int|void)\s+" + name + r"\s*\(", src)
    assert hasattr(ctypes.CDLL(ope.LIB_PATH), name)
    assert name in {n for n, _, _ in ope.ABI}


def test_track_layouts_match_the_c_compiler(ope):
    structs = {ope.TrackParams: "ope_track_params", ope.TrackCentroid: "ope_track_centroid", ope.TrackGateResult: "ope_track_gate_result",
               ope.TrackResult: "ope_track_result"}
    got = ctypes_layout(structs)
    got.update({"b.none": ope.TRACK_NO_CLUSTERS, "b.gated": ope.TRACK_GATED, "b.all": ope.TRACK_REALIGN_ALL, "b.nothing": ope.TRACK_NOTHING,
                "b.loop": ope.TRACK_REALIGN_LOOP, "skipped": ope.TRACK_COARSE_SKIPPED})
    got["abi"] = 5   # the change only adds to the ABI
    assert got == c_layout(structs, extra={"b.none": "OPE_TRACK_NO_CLUSTERS", "b.gated": "OPE_TRACK_GATED", "b.all": "OPE_TRACK_REALIGN_ALL",
                                           "b.nothing": "OPE_TRACK_NOTHING", "b.loop": "OPE_TRACK_REALIGN_LOOP",
                                           "skipped": "OPE_TRACK_COARSE_SKIPPED", "abi": "OPE_ABI_VERSION"})


def test_track_defaults_are_the_reference_literals(ope):
    p = ope.default_track_params()
    assert p.gate_distance == 0.05          # "distance < 0.05" / "distance > 0.05" (rosinterface.cpp:279,304)
    assert p.coarse_fitness == 1e-4         # "fitnessScoreFine > 0.0001" (poseestimator.cpp:399)
    assert bytes(p.final) == bytes(ope.default_final_params())
    assert (p.final.accept_fitness, p.final.accept_strength) == (1e-4, 0.4)   # rosinterface.cpp:256
