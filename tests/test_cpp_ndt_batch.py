"""fast_gicp::LoopVerifierHip::setNDT (riv-slam_amd/cpp/loop_verifier_hip.hpp): NDT for loop verification from C++, compiled against
tests/pcl_shim (PCL is not installed here): tests/cpp/test_ndt_batch.cpp."""
import importlib
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "_build", "test_ndt_batch")


def build_exe():
    import __graft_entry__ as g
    g.build()
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    lib_dir = os.path.join(ROOT, "riv-slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "tests", "pcl_shim"), "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "riv-slam_amd", "cpp"), os.path.join(ROOT, "tests", "cpp", "test_ndt_batch.cpp"),
                           "-L", lib_dir, "-lapdgicp_hip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-o", EXE])
    return EXE


def test_cpp_verifier_with_setndt_compiles_and_links():
    out = subprocess.run([build_exe()], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.split() == ["compile-only", "0"], (out.stdout, out.stderr)


@pytest.mark.gpu
def test_cpp_verifier_picks_the_candidate_the_single_object_loop_picks(scene, tmp_path):
    """1 target x 6 candidates of 2048 points through LoopVerifierHip with setNDT(D2D, DIRECT7, resolution 2.0), and through the reference's
    loop over one NDTHip (align + getFitnessScore per candidate): the same candidate, the same converged flags, and every pose within
    1e-3 m / 1e-4 rad of the class's (iteration counts are compared where the face margin of the run is known: tests/test_ndt_batch.py);
    setVGICP after setNDT switches NDT off, and setNDT after that switches voxelized GICP off."""
    exe = build_exe()
    reg = importlib.import_module("riv-slam_amd.registration")
    # the new keyframe (the scan) is the TARGET, the six keyframes before it are the candidates (loop_detector.cpp:392-411)
    tgt, cands, _, to_keyframe = scene.make_keyframe_set(4099, 2048, 6, scene.pair_seed(7, 3))
    guesses = [np.linalg.inv(g.astype(np.float64)).astype(np.float32) for g in to_keyframe]
    path, outp = tmp_path / "set.bin", tmp_path / "out.bin"
    with open(path, "wb") as fh:
        np.array([len(cands), len(tgt), len(cands[0])], dtype=np.int32).tofile(fh)
        np.ascontiguousarray(np.stack([np.asarray(g, dtype=np.float32).T for g in guesses])).tofile(fh)   # column-major
        np.ascontiguousarray(tgt, dtype=np.float32).tofile(fh)
        for c in cands:
            np.ascontiguousarray(c, dtype=np.float32).tofile(fh)
    out = subprocess.run([exe, str(path), str(outp)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout, out.stderr)
    best_batch, best_loop, flags_equal, exclusive = (int(v) for v in out.stdout.split())
    assert best_batch == best_loop and flags_equal == 1 and exclusive == 1
    recs = np.fromfile(outp, dtype=reg.RESULT_DTYPE)
    assert len(recs) == 12
    for i in range(6):
        a, b = recs[i], recs[6 + i]
        assert int(a["converged"]) == int(b["converged"]) and int(a["lm_failed"]) == int(b["lm_failed"]) == 0, (i, a, b)
        te, re_ = scene.pose_error(b["T"].reshape(4, 4).T, a["T"].reshape(4, 4).T)
        assert te <= 1e-3 and re_ <= 1e-4
