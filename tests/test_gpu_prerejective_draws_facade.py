"""PoseEstimator::setCoarseDeviceDraws through the driver: `detect_and_localize --candidates --coarse prerejective --coarse-batch
--device-draws` prints the result lines of the same command without --device-draws (the draws are the same, so everything after
them is), and the flag is refused without the aligner and the batch it belongs to.  The files are those of
tests/test_gpu_prerejective_batch_facade.py."""
import subprocess

import numpy as np
import pytest

import test_gpu_prerejective_batch_facade as fac

pytestmark = pytest.mark.gpu

files = fac.files          # the module-scoped fixture: a distractor, 9 key points, the scene cluster, another distractor


def result_lines(rec):
    """Everything the driver printed but the path of the aligned cloud it wrote (a fresh temporary file per run)."""
    return [ln for ln in rec["stdout"].splitlines() if not ln.startswith("aligned ")]


def test_device_draws_print_the_same_result_lines(files):
    flags = ("--candidates", "--coarse", "prerejective", "--coarse-batch")
    host = fac.driver(files, *flags)
    dev = fac.driver(files, *flags, "--device-draws")
    assert "running the loop" not in dev["stderr"] and "running the loop" not in host["stderr"]      # the batched call was taken
    assert result_lines(dev) == result_lines(host)
    assert dev["coarse_calls"] >= 2 and dev["selected"] == host["selected"]
    assert dev["aligned"].tobytes() == host["aligned"].tobytes()
    print("[device draws driver]", dev["selected"], dev["fitness"], dev["strength"], dev["coarse_calls"], dev["icp_iterations"])


@pytest.mark.parametrize("flags", [("--candidates",), ("--candidates", "--coarse", "prerejective"), ("--candidates", "--coarse-batch"),
                                   ("--candidates", "--coarse", "correspondences", "--coarse-batch")],
                         ids=["alone", "without-the-batch", "with-sac-ia", "with-correspondences"])
def test_the_flag_alone_exits_2(files, flags):
    bad = subprocess.run([fac.EXE, *files, "--seed", "1", *flags, "--device-draws"], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2 and "--device-draws goes with --coarse prerejective --coarse-batch" in bad.stderr
    assert "candidates " not in bad.stdout


def test_the_flag_does_not_go_with_the_tracker(files):
    bad = subprocess.run([fac.EXE, "--track", fac.MODEL, "--device-draws", "--frame", files[3]], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2 and "--device-draws does not go with --track or --track-loop" in bad.stderr
