"""CPU-side checks of tracking (ope_track_gate, ope_track_pose): declared, exported and bound; the ctypes structs lay out
exactly as the C compiler lays out ope_track_params / ope_track_centroid / ope_track_gate_result / ope_track_result; the
defaults are the reference's literals (rosinterface.cpp:279,304, poseestimator.cpp:399)."""
import ctypes
import os
import re
import subprocess

import pytest

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


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "ope.h"
#define O(t, tag, m) printf("%s.%s %zu\n", tag, #m, offsetof(t, m))
int main(void) {
  printf("sizeof_p %zu\nsizeof_c %zu\nsizeof_g %zu\nsizeof_r %zu\n", sizeof(ope_track_params), sizeof(ope_track_centroid),
         sizeof(ope_track_gate_result), sizeof(ope_track_result));
  O(ope_track_params, "p", gate_distance); O(ope_track_params, "p", coarse_fitness); O(ope_track_params, "p", final);
  O(ope_track_centroid, "c", centroid); O(ope_track_centroid, "c", count); O(ope_track_centroid, "c", distance);
  O(ope_track_gate_result, "g", branch); O(ope_track_gate_result, "g", selected); O(ope_track_gate_result, "g", source);
  O(ope_track_result, "r", gate); O(ope_track_result, "r", selected); O(ope_track_result, "r", coarse_status);
  O(ope_track_result, "r", seed); O(ope_track_result, "r", coarse); O(ope_track_result, "r", fine); O(ope_track_result, "r", rigid);
  O(ope_track_result, "r", final_pose); O(ope_track_result, "r", icp); O(ope_track_result, "r", fitness);
  O(ope_track_result, "r", fitness_n); O(ope_track_result, "r", n_fine_src); O(ope_track_result, "r", n_fine_tgt);
  O(ope_track_result, "r", status); O(ope_track_result, "r", reserved);
  printf("b.none %d\nb.gated %d\nb.all %d\nb.nothing %d\nb.loop %d\nskipped %d\n", OPE_TRACK_NO_CLUSTERS, OPE_TRACK_GATED,
         OPE_TRACK_REALIGN_ALL, OPE_TRACK_NOTHING, OPE_TRACK_REALIGN_LOOP, OPE_TRACK_COARSE_SKIPPED);
  printf("abi %d\n", OPE_ABI_VERSION);
  return 0;
}
"""


def test_track_layouts_match_the_c_compiler(ope, tmp_path):
    c = tmp_path / "probe.c"
    c.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.check_call(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    want = dict(line.rsplit(" ", 1) for line in subprocess.check_output([str(exe)], text=True).splitlines())
    want = {k: int(v) for k, v in want.items()}
    structs = {"p": ope.TrackParams, "c": ope.TrackCentroid, "g": ope.TrackGateResult, "r": ope.TrackResult}
    got = {"sizeof_" + t: ctypes.sizeof(S) for t, S in structs.items()}
    for t, S in structs.items():
        for name, _ in S._fields_:
            got[t + "." + name] = getattr(S, name).offset
    got.update({"b.none": ope.TRACK_NO_CLUSTERS, "b.gated": ope.TRACK_GATED, "b.all": ope.TRACK_REALIGN_ALL, "b.nothing": ope.TRACK_NOTHING,
                "b.loop": ope.TRACK_REALIGN_LOOP, "skipped": ope.TRACK_COARSE_SKIPPED})
    got["abi"] = 5   # the change only adds to the ABI
    assert got == want


def test_track_defaults_are_the_reference_literals(ope):
    p = ope.default_track_params()
    assert p.gate_distance == 0.05          # "distance < 0.05" / "distance > 0.05" (rosinterface.cpp:279,304)
    assert p.coarse_fitness == 1e-4         # "fitnessScoreFine > 0.0001" (poseestimator.cpp:399)
    assert bytes(p.final) == bytes(ope.default_final_params())
    assert (p.final.accept_fitness, p.final.accept_strength) == (1e-4, 0.4)   # rosinterface.cpp:256
