"""radar_graph_slam::ScanFilterHip with setDownsampleMethod("APPROX_VOXELGRID") (riv-slam_amd/cpp/scan_filter_hip.hpp), compiled against
tests/pcl_shim (PCL is not installed here): tests/cpp/test_approx_voxel.cpp."""
import os
import subprocess

import numpy as np
import pytest

import approx_voxel_np as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "_build", "test_approx_voxel")


def build_exe():
    import __graft_entry__ as g
    g.build()
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    lib_dir = os.path.join(ROOT, "riv-slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "tests", "pcl_shim"), "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "riv-slam_amd", "cpp"), os.path.join(ROOT, "tests", "cpp", "test_approx_voxel.cpp"),
                           "-L", lib_dir, "-lapdgicp_hip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-o", EXE])
    return EXE


def test_cpp_class_compiles_links_and_knows_the_name():
    """the three documented names of downsample_method are taken without the "is not offered" warning"""
    out = subprocess.run([build_exe()], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "compile-only" in out.stdout
    assert "not offered" not in out.stderr, out.stderr


@pytest.mark.gpu
def test_cpp_class_gives_the_restatements_bytes(tmp_path):
    """The collision cloud (3 000 points, leaf 0.5: more outputs than voxels) written by this side, through the class with the gate off and
    no outlier filter: n_out and the checksum of the output bytes are the literal loop's."""
    exe = build_exe()
    cloud, leaf, want, ijk, _ = A.expected("collisions")
    assert len(want) > len(np.unique(ijk, axis=0))
    path = tmp_path / "scan.bin"
    with open(path, "wb") as fh:
        np.array([len(cloud)], dtype=np.int32).tofile(fh)
        cloud.tofile(fh)
    out = subprocess.run([exe, str(path), repr(float(leaf))], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert "not offered" not in out.stderr
    n_out, h = (int(v) for v in out.stdout.split())
    assert (n_out, h) == (len(want), A.checksum(want))
