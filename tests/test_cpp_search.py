"""The C++ drop-in class's search beyond k = 1 (riv-slam_amd/cpp/fast_apdgicp_hip.hpp): the batch nearestKSearch with k = 5 in one
device pass and deviceRadiusSearch, driven by tests/cpp/test_search_adapter.cpp against tests/pcl_shim."""
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "_build", "test_search_adapter")


def build_exe():
    import __graft_entry__ as g
    g.build()
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    lib_dir = os.path.join(ROOT, "riv-slam_amd")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "tests", "pcl_shim"), "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "riv-slam_amd", "cpp"), os.path.join(ROOT, "tests", "cpp", "test_search_adapter.cpp"),
           "-L", lib_dir, "-lapdgicp_hip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-o", EXE]
    subprocess.check_call(cmd)
    return EXE


def test_search_adapter_compiles_and_links():
    exe = build_exe()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "compile-only" in out.stdout


@pytest.mark.gpu
def test_batch_knn_and_radius_search_through_the_adapter(golden, tmp_path):
    """Batch nearestKSearch(cloud, indices, 5, ...): every row equals the host scan's (host_nn through the single-point call, and a scan
    written in the program), counted in device_queries with `fallbacks` unchanged; deviceRadiusSearch equals a host scan for r = 0 and
    r = 0.6 with max_nn = 0, 3 and one above the target's size; the registration afterwards is the one before."""
    exe = build_exe()
    src, tgt, guess = golden["lin_source"], golden["lin_target"], golden["lin_guess"]
    path = tmp_path / "pair.bin"
    with open(path, "wb") as f:
        np.array([len(src), len(tgt)], dtype=np.int32).tofile(f)
        np.asfortranarray(guess).T.astype(np.float32).tofile(f)
        src.astype(np.float32).tofile(f)
        tgt.astype(np.float32).tofile(f)
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    d = json.loads(out.stdout.strip().splitlines()[-1])
    assert d["converged"] == 1
    assert d["knn_vs_scan"] == 1 and d["knn_vs_host_nn"] == 1 and d["sub_ok"] == 1
    assert d["knn_fallbacks"] == 0 and d["knn_device_queries"] == d["n_queries"]
    assert d["single_fallbacks"] == d["n_queries"]            # the single-point k = 5 path is still the host scan
    assert d["radius_ok"] == 1 and d["radius_fallbacks"] == 0
    assert d["radius_rows_nonempty"] > 0 and d["radius_rows_cut"] > 0
    assert d["converged_after"] == 1 and d["same_iterations"] == 1
