"""The C++ class fast_gicp::FastGICPMultiPointsHip (riv-slam_amd/cpp/fast_gicp_mp_hip.hpp), compiled against tests/pcl_shim (PCL is not
installed here): tests/cpp/test_gicp_mp_adapter.cpp."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "_build", "test_gicp_mp_adapter")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gicp_mp_cases as cases  # noqa: E402


def build_exe():
    import __graft_entry__ as g
    g.build()
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    lib_dir = os.path.join(ROOT, "riv-slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "tests", "pcl_shim"), "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "riv-slam_amd", "cpp"), os.path.join(ROOT, "tests", "cpp", "test_gicp_mp_adapter.cpp"),
                           "-L", lib_dir, "-lapdgicp_hip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-o", EXE])
    return EXE


def test_cpp_class_compiles_links_and_has_the_class_defaults():
    out = subprocess.run([build_exe()], capture_output=True, text=True, timeout=120)
    # MP8: k 20, 64 iterations, both epsilons 1e-5, PLANE (3), radius 0.5
    assert out.returncode == 0 and out.stdout.split() == ["compile-only", "20", "64", "1e-05", "1e-05", "3", "0.5"], (out.stdout, out.stderr)


@pytest.mark.gpu
def test_cpp_class_equals_the_c_abi_and_the_python_class(tmp_path):
    """Through the class (32-byte pcl::PointXYZI, pcl::Registration base pointer) and through the C ABI (packed xyz): byte-equal
    apdgicp_result records, hasConverged, getFinalTransformation and getFitnessScore; the Python class's run gives the same record."""
    exe = build_exe()
    reg = importlib.import_module("riv-slam_amd.registration")
    gmp = importlib.import_module("riv-slam_amd.gicp_mp")
    src, tgt, guess, radius = cases.scene_pair("converged_r2.0")
    path, outp = tmp_path / "pair.bin", tmp_path / "out.bin"
    with open(path, "wb") as fh:
        np.array([len(src), len(tgt)], dtype=np.int32).tofile(fh)
        np.ascontiguousarray(guess.T, dtype=np.float32).tofile(fh)   # column-major
        np.array([radius], dtype=np.float64).tofile(fh)
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
    g = gmp.FastGICPMultiPoints()
    g.setNeighborSearchRadius(radius)
    g.setInputSource(src)
    g.setInputTarget(tgt)
    g.align(guess)
    assert bytes(g.result) == recs[0].tobytes()
    assert (converged, iterations, state) == (int(g.hasConverged()), g.nr_iterations, g.state()) == (1, iterations, gmp.CONVERGED)
    assert g.getFitnessScore() == fits[0]
    g.close()
