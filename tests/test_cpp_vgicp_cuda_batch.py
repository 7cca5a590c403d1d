"""fast_gicp::LoopVerifierHip::setVGICPCuda (riv-slam_amd/cpp/loop_verifier_hip.hpp): FAST_VGICP_CUDA for loop verification from C++, through
the C ABI (tests/cpp/test_vgicp_cuda_batch.cpp).  The records must be the bytes the Python path (BatchVGICPCuda through
loop_verifier.verify_candidates) gets for the same clouds."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import vgicp_cuda_batch_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "_build", "test_vgicp_cuda_batch")


def build_exe():
    import __graft_entry__ as g
    g.build()
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    lib_dir = os.path.join(ROOT, "riv-slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "riv-slam_amd", "cpp"),
                           os.path.join(ROOT, "tests", "cpp", "test_vgicp_cuda_batch.cpp"), "-L", lib_dir, "-lapdgicp_hip", f"-Wl,-rpath,{lib_dir}",
                           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-o", EXE])
    return EXE


def test_cpp_verifier_with_setvgicpcuda_compiles_and_links():
    out = subprocess.run([build_exe()], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.split() == ["compile-only", "0"], (out.stdout, out.stderr)


@pytest.mark.gpu
def test_cpp_records_are_the_python_path_s_bytes(tmp_path):
    """The fixture's target x six candidates (source prefixes 2048 .. 65, each from its own guess) through LoopVerifierHip with
    setVGICPCuda(DIRECT_RADIUS 1.5) and through loop_verifier.verify_candidates with a BatchVGICPCuda: byte-identical records, the same
    scores, the same candidate; one wait prepared the seven clouds and one more built the one map."""
    exe = build_exe()
    reg = importlib.import_module("riv-slam_amd.registration")
    vc = importlib.import_module("riv-slam_amd.vgicp_cuda")
    lv = importlib.import_module("riv-slam_amd.loop_verifier")
    pair = K.load_pair()
    tgt, srcs = K.batch_clouds(pair)
    cands, guesses = srcs[:6], K.batch_guesses(pair)[:6]
    path, outp = tmp_path / "set.bin", tmp_path / "out.bin"
    with open(path, "wb") as fh:
        np.array([len(cands), len(tgt)] + [len(c) for c in cands], dtype=np.int32).tofile(fh)
        np.ascontiguousarray(np.stack([np.asarray(g, dtype=np.float32).T for g in guesses])).tofile(fh)   # column-major
        np.ascontiguousarray(tgt, dtype=np.float32).tofile(fh)
        for c in cands:
            np.ascontiguousarray(c, dtype=np.float32).tofile(fh)
    out = subprocess.run([exe, str(path), str(outp)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout, out.stderr)
    best, refused, others_off = (int(v) for v in out.stdout.split())
    raw = open(outp, "rb").read()
    nrec = 6 * reg.RESULT_DTYPE.itemsize
    recs = np.frombuffer(raw[:nrec], dtype=reg.RESULT_DTYPE)
    scores = np.frombuffer(raw[nrec:nrec + 48], dtype=np.float64)
    counts = np.frombuffer(raw[nrec + 48:], dtype=np.int64)
    b = vc.BatchVGICPCuda(reg.default_params())
    b.setNeighborSearchMethod(vc.DIRECT_RADIUS, 1.5)
    loop, py_scores, py_recs = lv.verify_candidates(b, tgt, cands, guesses, fitness_score_thresh=5.0)
    assert refused == 1 and others_off == 1
    assert recs.tobytes() == py_recs.tobytes()
    assert np.array_equal(scores, np.asarray(py_scores, dtype=np.float64))
    assert loop is not None and best == loop.candidate
    assert all(int(r["converged"]) == 1 for r in recs)
    assert counts.tolist() == [7, 1, 1, 1] and b.build_count() == (7, 1) and b.debug_counts()[:2] == (1, 1)
