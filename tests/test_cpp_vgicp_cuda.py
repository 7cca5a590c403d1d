"""The C++ class fast_gicp::FastVGICPCudaHip (riv-slam_amd/cpp/fast_vgicp_cuda_hip.hpp), compiled against tests/pcl_shim (PCL is not
installed here): tests/cpp/test_vgicp_cuda_adapter.cpp."""
import importlib
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "_build", "test_vgicp_cuda_adapter")


def build_exe():
    import __graft_entry__ as g
    g.build()
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    lib_dir = os.path.join(ROOT, "riv-slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "tests", "pcl_shim"), "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "riv-slam_amd", "cpp"), os.path.join(ROOT, "tests", "cpp", "test_vgicp_cuda_adapter.cpp"),
                           "-L", lib_dir, "-lapdgicp_hip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-o", EXE])
    return EXE


def test_cpp_class_compiles_and_links():
    out = subprocess.run([build_exe()], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.split() == ["compile-only", "3"], (out.stdout, out.stderr)   # PLANE


@pytest.mark.gpu
def test_cpp_class_equals_the_c_abi_and_the_python_path(tmp_path):
    """The setters (each accepted value read back, the no-op setCorrespondenceRandomness, five refused settings that keep the last accepted
    one), then DIRECT_RADIUS 1.5 through the class (32-byte pcl::PointXYZI, pcl::Registration base pointer) and through the C ABI (packed
    xyz): byte-equal apdgicp_result records, equal to the record of the Python path."""
    exe = build_exe()
    reg = importlib.import_module("riv-slam_amd.registration")
    vc = importlib.import_module("riv-slam_amd.vgicp_cuda")
    pair = dict(np.load(os.path.join(ROOT, "tests", "golden", "vgicp_cuda_pair.npz")))
    src, tgt, guess = pair["source"], pair["target"], pair["guess"]
    path, outp = tmp_path / "pair.bin", tmp_path / "out.bin"
    with open(path, "wb") as fh:
        np.array([len(src), len(tgt)], dtype=np.int32).tofile(fh)
        np.ascontiguousarray(guess.T, dtype=np.float32).tofile(fh)   # column-major
        src.tofile(fh)
        tgt.tofile(fh)
    out = subprocess.run([exe, str(path), str(outp)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout, out.stderr)
    equal, converged, iterations, voxels, kept_s, kept_t, setters = (int(v) for v in out.stdout.split())
    assert equal == 1 and setters == 1, (out.stdout, out.stderr)
    for refused in ("setNearestNeighborSearchMethod failed", "setRegularizationMethod failed", "setNeighborSearchMethod failed", "setResolution failed"):
        assert refused in out.stderr          # a refused setting says so
    recs = np.fromfile(outp, dtype=reg.RESULT_DTYPE)
    assert len(recs) == 2 and recs[0].tobytes() == recs[1].tobytes()
    g = vc.FastVGICPCuda(reg.default_params(transformation_epsilon=0.01))
    g.setNeighborSearchMethod(vc.DIRECT_RADIUS, 1.5)
    g.setInputSource(src)
    g.setInputTarget(tgt)
    g.align(guess)
    assert bytes(g.result) == recs[0].tobytes()
    assert (converged, iterations, voxels, kept_s, kept_t) == (int(g.result.converged), g.result.iterations, g.voxel_count(), len(g.kept(0)), len(g.kept(1)))
    assert kept_s == len(pair["source_kept"]) and kept_t == len(pair["target_kept"]) and g.result.n_matched > 300
