"""radar_graph_slam::ScanIngestHip::runPolar / histogramAdd / histogramLast / pointDistribution (riv-slam_amd/cpp/scan_ingest_hip.hpp),
compiled against tests/pcl_shim as tests/test_cpp_scan_ingest.py builds its program: tests/cpp/test_polar_ingest.cpp, with a 19-float
target structure of its own."""
import os
import struct
import subprocess

import numpy as np
import pytest

import polar_ingest_np as P
from test_polar_ingest import check_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "_build", "test_polar_ingest")
F32 = np.float32


def build_exe():
    import __graft_entry__ as g
    g.build()
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    lib_dir = os.path.join(ROOT, "riv-slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "tests", "pcl_shim"), "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "riv-slam_amd", "cpp"), os.path.join(ROOT, "tests", "cpp", "test_polar_ingest.cpp"),
                           "-L", lib_dir, "-lapdgicp_hip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-o", EXE])
    return EXE


def test_cpp_polar_methods_compile_and_link():
    out = subprocess.run([build_exe()], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "compile-only" in out.stdout


@pytest.mark.gpu
def test_cpp_class_equals_the_c_abi_and_the_restatement(tmp_path):
    """1 500 targets through the class (76-byte structures in, the rows as a pcl cloud into the histogram, twice) and through the C ABI
    called directly (the five lanes at their field offsets, the histogram from the device rows): the same bytes, and the restatement's
    under the bars of tests/test_polar_ingest.py."""
    exe = build_exe()
    lanes = P.fixture(1500, 41)
    rec = P.targets(*lanes)
    path, outp = tmp_path / "scan.bin", tmp_path / "out.bin"
    with open(path, "wb") as fh:
        fh.write(struct.pack("<i", len(rec)))
        rec.tofile(fh)
    out = subprocess.run([exe, str(path), str(outp)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    same, n_out = (int(v) for v in out.stdout.split())
    assert same == 1 and n_out == 1500
    blob = np.fromfile(outp, dtype=np.uint8)
    assert blob[:4].view(np.int32)[0] == n_out and len(blob) == 4 + 36 * n_out + 400 + 800
    at = 4
    rows = blob[at:at + 32 * n_out].view(F32).reshape(n_out, 8)
    at += 32 * n_out
    index = blob[at:at + 4 * n_out].view(np.int32)
    at += 4 * n_out
    counts = blob[at:at + 400].view(np.int32)
    dist = blob[at + 400:at + 1200].view(np.int64)
    check_rows(dict(rows=rows, index=index), lanes, "the C++ class")
    want = P.histogram(rows)
    assert np.array_equal(counts, want) and np.array_equal(dist, (2 * want.astype(np.int64)) // 2) and want.sum() > 0
