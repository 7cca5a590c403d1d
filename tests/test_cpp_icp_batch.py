"""fast_gicp::LoopVerifierHip::setICP (riv-slam_amd/cpp/loop_verifier_hip.hpp): point-to-point ICP for loop verification from C++, compiled
against tests/pcl_shim (PCL is not installed here): tests/cpp/test_icp_batch.cpp."""
import importlib
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "_build", "test_icp_batch")


def build_exe():
    import __graft_entry__ as g
    g.build()
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    lib_dir = os.path.join(ROOT, "riv-slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "tests", "pcl_shim"), "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "riv-slam_amd", "cpp"), os.path.join(ROOT, "tests", "cpp", "test_icp_batch.cpp"),
                           "-L", lib_dir, "-lapdgicp_hip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-o", EXE])
    return EXE


def test_cpp_verifier_with_seticp_compiles_and_links():
    out = subprocess.run([build_exe()], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.split() == ["compile-only", "0"], (out.stdout, out.stderr)


@pytest.mark.gpu
def test_cpp_verifier_records_equal_the_single_object_loop(scene, tmp_path):
    """1 target x 6 candidates of 2048 points through LoopVerifierHip with setICP (reciprocal, 10 iterations, epsilon 1e-5, gate 2.5 m), and
    through the reference's loop over one IterativeClosestPointHip (align + getFitnessScore per candidate): the same candidate, every
    record byte-equal (IC13), every state equal; each of setICP / setVGICP / setNDT switches the other two off."""
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
    best_batch, best_loop, records_equal, states_equal, exclusive = (int(v) for v in out.stdout.split())
    assert best_batch == best_loop and records_equal == 1 and states_equal == 1 and exclusive == 1
    recs = np.fromfile(outp, dtype=reg.RESULT_DTYPE)
    assert len(recs) == 12
    for i in range(6):
        assert recs[i].tobytes() == recs[6 + i].tobytes(), i
        assert int(recs[i]["iterations"]) >= 1 and int(recs[i]["n_matched"]) >= 3
