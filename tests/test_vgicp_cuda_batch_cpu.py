"""FAST_VGICP_CUDA as a mode of the BATCH handle, the part that needs no GPU: exports, the header's VC11 .. VC16, the Python class, the
argument checks that need no handle, and -- with the restatement tests/vgicp_cuda_np.py alone -- the two conditions under which
tests/test_vgicp_cuda_batch.py compares kept lists and integer record fields exactly, for every cloud and every pair it uses:
  * PLANE threshold margin > 1e-9 and gap margin >= 1e-6 (filter_conditions, the bars of test_fixture_meets_its_conditions);
  * face margin >= 1e-9 over the whole run (FACE_MARGIN of the existing tests), LM and GN, every search.
Which pairs converge is asserted here too: the GPU tests compare floats against the single handle for those only."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest

import vgicp_cuda_batch_cases as K
import vgicp_cuda_np as VC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("apdgicp_batch_set_vgicp_cuda", "apdgicp_batch_get_vgicp_cuda", "apdgicp_batch_vgicp_cuda_kept", "apdgicp_batch_vgicp_cuda_get_covariances",
               "apdgicp_batch_vgicp_cuda_voxel_count", "apdgicp_batch_vgicp_cuda_get_voxels", "apdgicp_batch_vgicp_cuda_get_correspondences",
               "apdgicp_batch_vgicp_cuda_build_count", "apdgicp_batch_vgicp_cuda_debug_counts", "apdgicp_batch_vgicp_cuda_last_phases")


@pytest.fixture(scope="module")
def reg():
    import __graft_entry__ as g
    g.build()
    return importlib.import_module("riv-slam_amd.registration")


@pytest.fixture(scope="module")
def vc(reg):
    return importlib.import_module("riv-slam_amd.vgicp_cuda")


@pytest.fixture(scope="module")
def pair():
    return K.load_pair()


@pytest.fixture(scope="module")
def prepared(pair):
    """the restatement's prepared clouds of the align batch, computed once: (target, [source k])"""
    tgt, srcs = K.batch_clouds(pair)
    return VC.prepare(tgt), [VC.prepare(s) for s in srcs]


def test_new_symbols_are_exported_declared_and_listed(reg, vc):
    L = reg.load_library()
    header = open(os.path.join(ROOT, "include", "apdgicp_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), f"{name} is not exported"
        assert name in reg.SYMBOLS
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared"
    for k in range(11, 17):
        assert f"VC{k}." in header
    assert "in this mode: not built" not in header
    assert L.apdgicp_abi_version() == 6
    loop_verifier = open(os.path.join(ROOT, "riv-slam_amd", "cpp", "loop_verifier_hip.hpp")).read()
    assert re.search(r"\bint setVGICPCuda\(const apdgicp_vgicp_cuda_params\*", loop_verifier)


def test_the_python_class(reg, vc):
    assert issubclass(vc.BatchVGICPCuda, reg.BatchAPDGICP)
    for m in ("setResolution", "setRegularizationMethod", "setNeighborSearchMethod", "setNearestNeighborSearchMethod", "setCorrespondenceRandomness", "enable", "disable",
              "enabled", "get_mode", "offsets", "kept", "covariances", "voxel_count", "voxels", "voxel_correspondences", "build_count", "align", "align_async",
              "synchronize", "fitness", "set_clouds"):
        assert callable(getattr(vc.BatchVGICPCuda, m)), m


def _params(vc, **kw):
    p = vc.default_vgicp_cuda_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("kw, code", [
    ({}, -1),                                                 # valid parameters reach the handle check: the handle is null
    (dict(neighbor_search=3, search_radius=4.0), -1),
    (dict(nn_method=2), -5),                                  # GPU_RBF_KERNEL
    (dict(regularization=0), -5),                             # NONE
    (dict(regularization=2), -5),                             # NORMALIZED_MIN_EIG
    (dict(resolution=0.0), -1),
    (dict(resolution=float("nan")), -1),
    (dict(neighbor_search=3, search_radius=4.5), -1),
    (dict(neighbor_search=3, search_radius=-0.5), -1),
])
def test_set_checks_its_parameters_before_the_handle(reg, vc, kw, code):
    L = reg.load_library()
    assert L.apdgicp_batch_set_vgicp_cuda(None, ctypes.byref(_params(vc, **kw))) == code
    if kw and code == -5:
        assert "FAST_VGICP_CUDA" in L.apdgicp_last_error().decode()
    if "resolution" in kw:
        assert "resolution" in L.apdgicp_last_error().decode()
    if kw.get("search_radius") in (4.5, -0.5):
        assert "radius" in L.apdgicp_last_error().decode()


def test_every_getter_refuses_a_null_handle(reg, vc):
    L = reg.load_library()
    n, m, t = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    buf = np.zeros(64, dtype=np.int32)
    p = ctypes.c_void_p(buf.ctypes.data)
    assert L.apdgicp_batch_set_vgicp_cuda(None, None) == -1
    assert L.apdgicp_batch_get_vgicp_cuda(None, None, None) == -1
    assert L.apdgicp_batch_vgicp_cuda_kept(None, 0, ctypes.byref(n), None, 0) == -1
    assert L.apdgicp_batch_vgicp_cuda_get_covariances(None, 0, None, None, 0) == -1
    assert L.apdgicp_batch_vgicp_cuda_voxel_count(None, 0, ctypes.byref(n)) == -1
    assert L.apdgicp_batch_vgicp_cuda_get_voxels(None, 0, 0, None, None, None, None) == -1
    assert L.apdgicp_batch_vgicp_cuda_get_correspondences(None, 0, p, 0) == -1
    assert L.apdgicp_batch_vgicp_cuda_get_correspondences(None, 0, None, 0) == -1
    assert L.apdgicp_batch_vgicp_cuda_build_count(None, ctypes.byref(n), ctypes.byref(m)) == -1
    assert L.apdgicp_batch_vgicp_cuda_last_phases(None, None) == -1
    assert L.apdgicp_batch_vgicp_cuda_debug_counts(None, ctypes.byref(n), ctypes.byref(m), ctypes.byref(t)) == -1


# ---------------------------------------------------------------------- the conditions behind the exact comparisons
def test_every_cloud_keeps_its_distance_from_the_plane_threshold(pair):
    clouds = [("target", n, pair["target"][:n]) for n in K.TARGET_PREFIXES] + [("source", n, pair["source"][:n]) for n in K.SOURCE_SIZES]
    clouds.append(("line", len(pair["line"]), pair["line"]))
    clouds.append(("refused target", 2078, K.refused_target(pair)))
    for name, n, cloud in clouds:
        c = VC.filter_conditions(VC.raw_covariances(cloud, VC.neighbours(cloud)))
        assert c["threshold_margin"] > 1e-9 and c["gap_margin"] >= 1e-6, (name, n, c)
    for n, kept in K.KEPT_SOURCE.items():
        assert len(VC.prepare(pair["source"][:n])["kept_index"]) == kept
    for n, kept in K.KEPT_TARGET.items():
        assert len(VC.prepare(pair["target"][:n])["kept_index"]) == kept
    assert len(VC.prepare(pair["line"])["kept_index"]) == 0
    # the refused target: PLANE keeps its first patch point, and has dropped points in front of it
    kept = VC.prepare(K.refused_target(pair))["kept_index"]
    assert 2048 in kept and int(np.nonzero(kept == 2048)[0][0]) < 2048


@pytest.mark.parametrize("optimizer", (0, 1), ids=("lm", "gn"))
@pytest.mark.parametrize("tag", [s[0] for s in K.SEARCHES])
def test_align_batches_keep_their_distance_from_the_voxel_faces(pair, prepared, tag, optimizer):
    """Every pair of the seven-pair batch (and of the loop-verification set, its first six pairs), whether it converges or not."""
    _, search, radius = next(s for s in K.SEARCHES if s[0] == tag)
    pt, ps = prepared
    guesses = K.batch_guesses(pair)
    iterations, converged = set(), []
    for k, n in enumerate(K.SOURCE_SIZES):
        o = K.restatement(ps[k], pt, search, radius, optimizer=optimizer)
        o.align(guesses[k])
        assert o.face_margin_min >= K.FACE_MARGIN, (n, o.face_margin_min)
        iterations.add(o.nr_iterations)
        if o.converged:
            converged.append(n)
    assert tuple(converged) == K.CONVERGING[tag]
    assert len(iterations) >= 2      # the pairs of a batch do not all finish in the same tick


@pytest.mark.parametrize("tag", [s[0] for s in K.FIRST_LINEARIZE_SEARCHES])
def test_first_linearize_keeps_its_distance_from_the_voxel_faces(pair, prepared, tag):
    _, search, radius = next(s for s in K.FIRST_LINEARIZE_SEARCHES if s[0] == tag)
    pt, ps = prepared
    guesses = K.batch_guesses(pair)
    for k, n in enumerate(K.SOURCE_SIZES):
        if tag == "r4.0" and n not in K.R4_SIZES:
            continue
        o = K.restatement(ps[k], pt, search, radius)
        o.update_correspondences(guesses[k].astype(np.float64))
        assert o.face_margin >= K.FACE_MARGIN and o.n_matched > 0, (n, o.face_margin)


def test_degenerate_and_small_pairs_keep_their_distance_too(pair, prepared):
    """The pairs of the GPU tests that are not in the seven-pair batch: a source against the 1024-point target (the too-few-points test's
    second align) and a source of 20 .. 29 points, fewer than the default k_correspondences."""
    pt, ps = prepared
    guesses = K.batch_guesses(pair)
    small_t = VC.prepare(pair["target"][:1024])
    for optimizer in (0, 1):
        for k in (3, 6):
            o = K.restatement(ps[k], small_t, VC.DIRECT7, 1.5, optimizer=optimizer)
            o.align(guesses[k])
            assert o.face_margin_min >= K.FACE_MARGIN
