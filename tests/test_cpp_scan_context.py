"""The C++ class radar_graph_slam::SCManagerHip (riv-slam_amd/cpp/scan_context_hip.hpp), compiled against tests/pcl_shim (PCL is not
installed here): tests/cpp/test_scan_context.cpp."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import scan_context_np as snp
from scan_context_np import fov_cloud
from test_scan_context import KNOBS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "_build", "test_scan_context")


def build_exe():
    import __graft_entry__ as g
    g.build()
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    lib_dir = os.path.join(ROOT, "riv-slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "tests", "pcl_shim"), "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "riv-slam_amd", "cpp"), os.path.join(ROOT, "tests", "cpp", "test_scan_context.cpp"),
                           "-L", lib_dir, "-lapdgicp_hip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-o", EXE])
    return EXE


def test_cpp_class_compiles_and_links():
    out = subprocess.run([build_exe()], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "compile-only" in out.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", list(KNOBS))
def test_cpp_class_equals_the_c_abi_and_the_restatement(knobs, tmp_path):
    """40 keyframes (one empty, one with a NaN point) through the class (32-byte pcl::PointXYZI) and through the C ABI called directly
    (16-byte rows): byte-equal records, and equal to the restatement"""
    scm = importlib.import_module("riv-slam_amd.scan_context")
    exe = build_exe()
    rng = np.random.default_rng(21)
    base = [fov_cloud(rng, 400) for _ in range(8)]
    clouds = []
    for k in range(40):     # eight places, seen again with noise
        c = base[k % 8].copy()
        c[:, :2] += rng.normal(size=(len(c), 2)).astype(np.float32) * 0.05
        clouds.append(c[: int(rng.integers(200, 401))])
    clouds[3] = np.zeros((0, 4), dtype=np.float32)
    clouds[5][7, 0] = np.nan
    query, top_k = 39, 6
    cand = rng.permutation(39).astype(np.int32)
    path, outp = tmp_path / "sc.bin", tmp_path / "out.bin"
    with open(path, "wb") as fh:
        np.array([len(clouds)], dtype=np.int32).tofile(fh)
        for c in clouds:
            np.array([len(c)], dtype=np.int32).tofile(fh)
            c.tofile(fh)
        np.array([query, top_k, len(cand)], dtype=np.int32).tofile(fh)
        cand.tofile(fh)
    kn = KNOBS[knobs]
    out = subprocess.run([exe, str(path), str(outp), str(kn["num_candidates"]), repr(kn["search_ratio"])], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    equal, n_out, loop = (int(v) for v in out.stdout.split())
    assert equal == 1
    ref = snp.ScanContextNP(**kn)
    for c in clouds:
        ref.add(c)
    want = ref.detect(query, cand, top_k)
    raw = np.fromfile(outp, dtype=np.uint8)
    n = int(raw[:4].view(np.int32)[0])
    got = raw[4:4 + 24 * n].view(scm.MATCH_DTYPE)
    assert n == n_out == len(want["matches"]) and loop == want["loop_id"] == 7      # keyframe 39 sees place 7 again
    assert got.tobytes() == snp.matches_array(want["matches"], scm.MATCH_DTYPE).tobytes()
    tail = raw[4 + 24 * n:]
    assert int(tail[:4].view(np.int32)[0]) == want["loop_id"] and tail[4:8].view(np.uint32)[0] == np.array([want["yaw"]], dtype=np.float32).view(np.uint32)[0]
