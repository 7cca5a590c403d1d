"""The C++ class pcl::IterativeClosestPointHip (riv-slam_amd/cpp/icp_hip.hpp), compiled against tests/pcl_shim (PCL is not installed
here): tests/cpp/test_icp_adapter.cpp."""
import importlib
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "_build", "test_icp_adapter")


def build_exe():
    import __graft_entry__ as g
    g.build()
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    lib_dir = os.path.join(ROOT, "riv-slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "tests", "pcl_shim"), "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "riv-slam_amd", "cpp"), os.path.join(ROOT, "tests", "cpp", "test_icp_adapter.cpp"),
                           "-L", lib_dir, "-lapdgicp_hip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-o", EXE])
    return EXE


def test_cpp_class_compiles_links_and_has_pcls_defaults():
    out = subprocess.run([build_exe()], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.split() == ["compile-only", "10", "0", "1", "3"], (out.stdout, out.stderr)   # 10 iterations, epsilon 0, no gate


@pytest.mark.gpu
def test_cpp_class_equals_the_c_abi(scene, tmp_path):
    """Reciprocal ICP through the class (32-byte pcl::PointXYZI, pcl::Registration base pointer) and through the C ABI (packed xyz):
    byte-equal apdgicp_result records, hasConverged, getFinalTransformation and getFitnessScore; and the Python wrapper's run of the
    same settings gives the same record."""
    exe = build_exe()
    reg = importlib.import_module("riv-slam_amd.registration")
    icp = importlib.import_module("riv-slam_amd.icp")
    src, tgt, _, guess = scene.make_pair(1500, 1700, scene.pair_seed(73, 0), "odometry")
    path, outp = tmp_path / "pair.bin", tmp_path / "out.bin"
    with open(path, "wb") as fh:
        np.array([len(src), len(tgt)], dtype=np.int32).tofile(fh)
        np.ascontiguousarray(guess.T, dtype=np.float32).tofile(fh)   # column-major
        src.tofile(fh)
        tgt.tofile(fh)
    out = subprocess.run([exe, str(path), str(outp)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout, out.stderr)
    equal, converged, iterations, state, same_T = (int(v) for v in out.stdout.split())
    assert equal == 1 and same_T == 1
    raw = open(outp, "rb").read()
    rs = reg.RESULT_DTYPE.itemsize
    recs = np.frombuffer(raw[:2 * rs], dtype=reg.RESULT_DTYPE)
    fits = np.frombuffer(raw[2 * rs:], dtype=np.float64)
    assert recs[0].tobytes() == recs[1].tobytes() and len(fits) == 2 and fits[0] == fits[1] and 0.0 < fits[0] < 10.0
    g = icp.ICP(icp.pcl_params(max_correspondence_distance=2.5, transformation_epsilon=1e-8, max_iterations=6), device=0)
    g.setUseReciprocalCorrespondences(True)
    g.setTransformationRotationEpsilon(2.0)
    g.setEuclideanFitnessEpsilon(1e-9)
    g.setInputSource(src)
    g.setInputTarget(tgt)
    g.align(guess)
    assert bytes(g.result) == recs[0].tobytes()
    assert (converged, iterations, state) == (int(g.hasConverged()), g.nr_iterations, g.convergence_state())
    assert g.getFitnessScore() == fits[0]
    g.close()
