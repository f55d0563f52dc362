"""PoseEstimator::setCorrespondencesBatch through the driver: `detect_and_localize --candidates --coarse correspondences
--correspondences-batch` (one ope_final_pose_batch_correspondences call) against `--candidates-loop --coarse correspondences` (one
estimateFinalPose at a time), with the fields and tolerances of tests/test_gpu_prerejective_batch_facade.py; without the flag the
driver prints what it printed before; the flag without --coarse correspondences is refused."""
import importlib
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

pcd = importlib.import_module("object-pose-estimation_amd.pcd")
synth = importlib.import_module("object-pose-estimation_amd.synth")
EXE = os.path.join(ROOT, "object-pose-estimation_amd", "build", "detect_and_localize")
GOLD = os.path.join(ROOT, "tests", "golden")
MODEL = os.path.join(GOLD, "drill_model_decimated.pcd")


def frob(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - np.asarray(b, np.float64)))


def driver(files, *flags):
    r = subprocess.run([EXE, *files, "--seed", "1", *flags], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    cand = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("candidates ")]
    frames = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("frame ")]
    assert len(cand) == 1 and len(frames) == 1, r.stdout
    tok = frames[0]
    rec = {"selected": int(cand[0][2]), "fitness": float(tok[3]), "strength": float(tok[5]), "coarse_calls": int(tok[7]),
           "icp_iterations": int(tok[9]), "stderr": r.stderr, "stdout": r.stdout}
    i = 10
    for name in ("final", "coarse", "fine", "rigid"):
        assert tok[i] == name
        rec[name + "_text"] = " ".join(tok[i + 1:i + 17])
        rec[name] = np.array([float(v) for v in tok[i + 1:i + 17]]).reshape(4, 4).T
        i += 17
    aligned = [ln.split(None, 1)[1] for ln in r.stdout.splitlines() if ln.startswith("aligned ")][0]
    rec["aligned"] = pcd.read_pcd(aligned)[0]
    return rec


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """A distractor, a cloud of 9 key points (no coarse call), the C1 scene cluster, another distractor."""
    tmp = tmp_path_factory.mktemp("corr_sac_batch_driver")
    scene = np.ascontiguousarray(np.load(os.path.join(GOLD, "drill_scene_c1.npz"))["scene"], np.float32)
    c = scene.mean(0)

    def blob(seed, at, scale):
        d = synth.model_surface(4000, seed=100 + seed) * np.float32(scale)
        return (d - d.mean(0) + np.asarray(at, np.float32)).astype(np.float32)

    tiny = scene[::200][:9] + np.arange(9, dtype=np.float32)[:, None] * np.float32(0.02)
    clouds = [blob(1, c + [0.25, 0.0, 0.0], 0.8), tiny, scene, blob(2, c + [-0.22, 0.1, 0.0], 1.1)]
    paths = [MODEL]
    for j, cl in enumerate(clouds):
        paths.append(str(tmp / f"cluster{j}.pcd"))
        pcd.write_pcd(paths[-1], cl.astype(np.float32))
    return paths


@pytest.fixture(scope="module")
def runs(files):
    return dict(batch=driver(files, "--candidates", "--coarse", "correspondences", "--correspondences-batch"),
                loop=driver(files, "--candidates-loop", "--coarse", "correspondences"),
                plain=driver(files, "--candidates", "--coarse", "correspondences"))


def test_correspondences_batch_matches_the_loop_of_estimate_final_pose(runs):
    one, loop = runs["batch"], runs["loop"]
    print("[correspondences batch driver]", one["selected"], one["fitness"], one["strength"], one["coarse_calls"], one["icp_iterations"])
    assert "running the loop" not in one["stderr"]                           # the batched call was taken, not its fallback
    assert one["selected"] == loop["selected"]
    assert one["coarse_calls"] == loop["coarse_calls"] >= 2 and one["icp_iterations"] == loop["icp_iterations"]
    assert abs(one["fitness"] - loop["fitness"]) <= 1e-6 * abs(loop["fitness"])
    for name in ("final", "coarse", "fine", "rigid"):
        assert frob(one[name], loop[name]) < 1e-4, (name, frob(one[name], loop[name]))
    assert one["aligned"].shape == loop["aligned"].shape and np.abs(one["aligned"] - loop["aligned"]).max() < 1e-4


def test_without_the_flag_the_driver_prints_what_it_printed_before(files, runs):
    plain, loop = runs["plain"], runs["loop"]
    for name in ("final", "coarse", "fine", "rigid"):
        assert plain[name + "_text"] == loop[name + "_text"], name             # the loop's poses, digit for digit
    assert (plain["selected"], plain["coarse_calls"], plain["icp_iterations"]) == (loop["selected"], loop["coarse_calls"], loop["icp_iterations"])
    # --coarse-batch keeps meaning what it meant: with this aligner the loop still runs
    cb = driver(files, "--candidates", "--coarse", "correspondences", "--coarse-batch")
    assert [cb[n + "_text"] for n in ("final", "coarse", "fine", "rigid")] == [loop[n + "_text"] for n in ("final", "coarse", "fine", "rigid")]


def test_the_flag_needs_the_correspondence_aligner(files):
    for extra in ([], ["--coarse", "prerejective"], ["--coarse", "sac-ia"]):
        bad = subprocess.run([EXE, *files, "--candidates", "--correspondences-batch", *extra], capture_output=True, text=True, timeout=60)
        assert bad.returncode == 2 and "--coarse correspondences" in bad.stderr
    bad = subprocess.run([EXE, "--track", MODEL, "--coarse", "correspondences", "--correspondences-batch", "--frame", files[3]],
                         capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2
