"""The C++ class DBSCANClusterHip<PointT> (riv-slam_amd/cpp/dbscan_hip.hpp), compiled against tests/pcl_shim (PCL is not installed here):
tests/cpp/test_dbscan.cpp."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import dbscan_np as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "_build", "test_dbscan")


def build_exe():
    import __graft_entry__ as g
    g.build()
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    lib_dir = os.path.join(ROOT, "riv-slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "tests", "pcl_shim"), "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "riv-slam_amd", "cpp"), os.path.join(ROOT, "tests", "cpp", "test_dbscan.cpp"),
                           "-L", lib_dir, "-lapdgicp_hip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-o", EXE])
    return EXE


def test_cpp_class_compiles_and_links():
    out = subprocess.run([build_exe()], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "compile-only" in out.stdout


@pytest.mark.gpu
def test_cpp_class_equals_the_c_abi_and_the_restatement(tmp_path):
    """900 points (blobs, noise, a NaN row, the D5 fixture far away) through the class (32-byte pcl::PointXYZI) and through the C ABI called
    directly (16-byte rows): byte-equal labels, CSR and table, and equal to the restatement"""
    db = importlib.import_module("riv-slam_amd.dbscan")
    exe = build_exe()
    rng = np.random.default_rng(23)
    centres = rng.uniform(-8, 8, (8, 3))
    pts = np.concatenate([c + 0.25 * rng.normal(size=(90, 3)) for c in centres] + [rng.uniform(-10, 10, (170, 3))])
    pts = pts[rng.permutation(len(pts))]
    quirk = np.zeros((9, 3))
    quirk[:, 0] = [0, 0.25, 0.5, 0.75, 1.25, 1.75, 2.0, 2.25, 2.5]
    quirk = quirk * (0.4 / 0.5) + 50.0        # the seed-quirk fixture scaled to eps 0.4 (exact in binary: x 0.8 is not, so the restatement decides)
    cloud = np.concatenate([pts, quirk, np.zeros((1, 3))]).astype(np.float32)
    cloud[100, 1] = np.nan
    xyzi = np.concatenate([cloud, rng.random((len(cloud), 1)).astype(np.float32)], axis=1)
    eps, min_pts, min_sz, max_sz = 0.4, 4, 5, 200
    path, outp = tmp_path / "cloud.bin", tmp_path / "out.bin"
    with open(path, "wb") as fh:
        np.array([len(xyzi)], dtype=np.int32).tofile(fh)
        np.ascontiguousarray(xyzi).tofile(fh)
    out = subprocess.run([exe, str(path), str(outp), repr(eps), str(min_pts), str(min_sz), str(max_sz)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    same, K = (int(v) for v in out.stdout.split())
    ref = D.extract(cloud, eps, min_pts=min_pts, min_cluster_size=min_sz, max_cluster_size=max_sz)
    want = D.table(cloud, ref, ref["core"])
    assert same == 1 and K == len(ref["clusters"]) >= 8
    raw = np.fromfile(outp, dtype=np.uint8)
    n = len(cloud)
    K2, M = (int(v) for v in raw[:8].view(np.int32))
    at = 8
    labels = raw[at:at + 4 * n].view(np.int32)
    at += 4 * n
    off = raw[at:at + 4 * (K + 1)].view(np.int32)
    at += 4 * (K + 1)
    idx = raw[at:at + 4 * M].view(np.int32)
    at += 4 * M
    table = raw[at:at + 80 * K].view(db.CLUSTER_DTYPE)
    assert K2 == K and at + 80 * K == len(raw)
    assert np.array_equal(labels, ref["labels"]) and np.array_equal(off, np.concatenate([[0], np.cumsum([len(c) for c in ref["clusters"]])]))
    assert np.array_equal(idx, np.concatenate(ref["clusters"]))
    assert np.array_equal(table["seed"], want["seed"]) and np.array_equal(table["size"], want["size"]) and np.array_equal(table["n_core"], want["n_core"])
    assert table["min"].tobytes() == want["min"].tobytes() and table["max"].tobytes() == want["max"].tobytes()
    for r, m in enumerate(ref["clusters"]):
        assert (np.abs(table["centroid"][r] - want["centroid"][r]) <= len(m) * 2.0**-52 * np.abs(cloud[m]).max(axis=0)).all()
