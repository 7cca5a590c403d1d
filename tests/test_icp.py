"""Point-to-point ICP as a mode of the registration handle: include/apdgicp_hip.h IC1 .. IC10, riv-slam_amd/csrc/apd_icp.hpp,
riv-slam_amd/icp.py, against the restatement tests/icp_np.py.

CPU part: exports, defaults, self-checks of the restatement against its second form.  GPU part (-m gpu): the per-iteration probe, the
reciprocal search, the gate, teacher-forced traces, every convergence state, free runs, the mode rules, determinism.

Bars: matches, fp32 distances and counts exact; mse 1e-12 relative; the 16 sums 1e-10 of their Frobenius norm; every element of a T_k
within one fp32 ulp (the fp64 SVDs differ near 1e-15, so only a value on a rounding boundary can move, and then by one ulp); W and the
fp32 product of IC6 bit for bit; free runs 1e-3 m / 1e-4 rad with state, iteration count and n_matched equal, asserted only where the
restatement alone shows a margin (no convergence quantity within 1e-3 relative of its threshold, no best and second-best distance
within 4 fp32 ulps).
"""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest

import icp_np as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("apdgicp_icp_default_params", "apdgicp_set_icp", "apdgicp_get_icp", "apdgicp_icp_estimate", "apdgicp_icp_get_correspondences",
               "apdgicp_icp_get_working_cloud", "apdgicp_icp_get_trace", "apdgicp_icp_convergence_state")
GATE = 2.5
DBL_MAX = float(np.finfo(np.float64).max)
f32 = np.float32


@pytest.fixture(scope="module")
def reg():
    import __graft_entry__ as g
    g.build()
    return importlib.import_module("riv-slam_amd.registration")


@pytest.fixture(scope="module")
def icp(reg):
    return importlib.import_module("riv-slam_amd.icp")


@pytest.fixture(scope="module")
def odo(scene):
    """The 2 048 x 2 048 odometry pair every small test cuts its clouds from, and three poses."""
    src, tgt, T_true, guess = scene.make_pair(2048, 2048, 20241023, "odometry")
    third = (scene.make_transform([0.05, -0.03, 0.02], 0.004, -0.003, 0.002) @ guess.astype(np.float64)).astype(f32)
    return src, tgt, T_true, guess, (np.eye(4, dtype=f32), guess.astype(f32), third)


def rigid_copy(scene, n, seed, t=(0.05, -0.02, 0.01), ypr=(0.004, -0.002, 0.003)):
    """A noise-free rigid copy at a small motion: (source, target = T * source in fp64 rounded to fp32, T)."""
    rng = np.random.default_rng(seed)
    src = (rng.uniform(-1, 1, size=(n, 3)) * [30, 30, 4]).astype(f32)
    T = scene.make_transform(t, *ypr)
    tgt = (src.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(f32)
    return src, tgt, T


# ====================================================================== CPU
def test_new_symbols_are_exported_and_the_module_imports(reg, icp):
    L = reg.load_library()
    header = open(os.path.join(ROOT, "include", "apdgicp_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), f"{name} is not exported"
        assert name in reg.SYMBOLS
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared"
    for name in ("ICP", "IcpParams", "default_icp_params"):
        assert hasattr(icp, name)
    for m in ("setUseReciprocalCorrespondences", "setEuclideanFitnessEpsilon", "setTransformationRotationEpsilon", "estimate", "correspondences",
              "working_cloud", "trace", "convergence_state", "align", "setInputSource", "setInputTarget"):
        assert callable(getattr(icp.ICP, m))
    assert issubclass(icp.ICP, reg.FastAPDGICP)
    assert L.apdgicp_abi_version() == 6
    for i in range(1, 11):
        assert re.search(r"\bIC%d\. " % i, header), f"IC{i} is missing from the header"
    assert "PCL 1.10" in header


def test_default_icp_params(icp):
    p = icp.default_icp_params()
    assert (p.enable, p.use_reciprocal_correspondences, p.min_correspondences, p.max_similar_transforms) == (1, 0, 3, 0)
    assert p.euclidean_fitness_epsilon == -DBL_MAX and p.rotation_epsilon == 0.0 and p.mse_threshold_absolute == 1e-12
    assert ctypes.sizeof(icp.IcpParams) == 40
    q = icp.pcl_params()
    assert q.max_iterations == 10 and q.transformation_epsilon == 0.0 and q.max_correspondence_distance ** 2 <= DBL_MAX
    assert tuple(range(6)) == (icp.NOT_CONVERGED, icp.ITERATIONS, icp.TRANSFORM, icp.ABS_MSE, icp.REL_MSE, icp.NO_CORRESPONDENCES)
    assert (I.NOT_CONVERGED, I.ITERATIONS, I.TRANSFORM, I.ABS_MSE, I.REL_MSE, I.NO_CORRESPONDENCES) == tuple(range(6))


def test_cpu_side_of_the_mode_rules(reg):
    """What needs no device: null handles and null outputs are refused with the codes of the header."""
    L = reg.load_library()
    p = ctypes.create_string_buffer(40)
    L.apdgicp_icp_default_params(None)   # accepted, like the other *_default_params
    assert L.apdgicp_set_icp(None, p) == -1 and L.apdgicp_get_icp(None, p, None) == -1
    assert L.apdgicp_icp_estimate(None, None, None, None, None, None) == -1
    assert L.apdgicp_icp_get_correspondences(None, None, None, 0) == -1
    assert L.apdgicp_icp_get_working_cloud(None, None, 0) == -1
    assert L.apdgicp_icp_get_trace(None, 0, None, None, None, None, None) == -1
    assert L.apdgicp_icp_convergence_state(None, None) == -1
    assert b"null" in L.apdgicp_last_error()


@pytest.mark.parametrize("seed", (3, 4, 5))
def test_restatement_agrees_with_its_second_form(scene, seed):
    """Tie-free fixtures: identical matches, T_k to 1e-12."""
    src, tgt, _, guess = scene.make_pair(600, 700, scene.pair_seed(70, seed), "odometry")
    W = I.working_cloud0(guess, src)
    match, d2, second = I.correspondences(W, tgt, GATE, want_second=True)
    assert np.all(second[np.isfinite(d2)] > d2[np.isfinite(d2)]), "the fixture has a tie"
    est = I.estimate(W, tgt, match, d2)
    m2, T2 = I.second_form_estimate(W, tgt, GATE)
    assert np.array_equal(match, m2) and est["n_corr"] == np.count_nonzero(m2 >= 0) > 300
    k = match >= 0
    R, t, *_ = I.umeyama(W[k], tgt[match[k]])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    assert np.abs(T - T2).max() <= 1e-12
    assert np.allclose(R @ R.T, np.eye(3), atol=1e-14) and np.linalg.det(R) > 0
    assert np.array_equal(est["T_k"], T.astype(f32))


def test_restatement_recovers_a_rigid_copy_in_one_estimate(scene):
    src, tgt, T = rigid_copy(scene, 500, 7)
    match, d2 = I.correspondences(src, tgt, 1.0)
    assert np.array_equal(match, np.arange(500))   # the motion is far below the point spacing
    est = I.estimate(src, tgt, match, d2)
    assert np.abs(est["T_k"].astype(np.float64) - T).max() <= 1e-6
    # reciprocity changes nothing on a one-to-one fixture, and removes the later of two duplicates that share a target
    assert np.array_equal(I.correspondences(src, tgt, 1.0, reciprocal=True)[0], match)
    dup = np.concatenate([src[:50], src[:50]])
    m = I.correspondences(dup, tgt, 1.0, reciprocal=True)[0]
    assert np.array_equal(m[:50], np.arange(50)) and np.all(m[50:] == -1)


def test_restatement_criteria_and_product():
    c = I.Criteria(5, 0.01)
    T = np.eye(4, dtype=f32)
    assert c(1, T, 1.0) and c.state == I.TRANSFORM
    c = I.Criteria(5, 0.01, max_similar=2)
    assert not c(1, T, 1.0) and c.similar == 1 and not c(2, T, 2.0) and c.similar == 2 and c(3, T, 3.0) and c.state == I.TRANSFORM
    c = I.Criteria(2, 1e-8, rotation_epsilon=2.0)
    assert not c(1, T, 1.0) and c(2, T, 0.5) and c.state == I.ITERATIONS
    c = I.Criteria(9, 1e-8, rotation_epsilon=2.0)
    assert not c(1, T, 1.0) and c(2, T, 1.0) and c.state == I.ABS_MSE
    c = I.Criteria(9, 1e-8, rotation_epsilon=2.0, mse_rel=0.5)
    assert not c(1, T, 1.0) and c(2, T, 0.75) and c.state == I.REL_MSE
    A = np.arange(16, dtype=f32).reshape(4, 4) / 7
    assert np.allclose(I.mul4(A, A.T), A.astype(np.float64) @ A.T.astype(np.float64), rtol=1e-6)


# ====================================================================== GPU
def make(icp, reg, src, tgt, device_input=False, linear=False, **kw):
    g = icp.ICP(icp.pcl_params(max_correspondence_distance=GATE, **kw), device=0)
    if linear:
        g.setTransformOrder(True)
    set_clouds(g, src, tgt, device_input)
    return g


def set_clouds(g, src, tgt, device_input=False):
    if device_input:
        import torch
        g.setInputSource(torch.from_numpy(np.ascontiguousarray(src)).cuda())
        g.setInputTarget(torch.from_numpy(np.ascontiguousarray(tgt)).cuda())
    else:
        g.setInputSource(src)
        g.setInputTarget(tgt)


def check_estimate(g, src, tgt, T, linear, reciprocal, what):
    """One probe against the restatement: the bars of the module docstring."""
    W = I.working_cloud0(T, src, linear)
    want = I.iterate(W, tgt, GATE, reciprocal)
    got = g.estimate(T)
    match, sq = g.correspondences()
    assert np.array_equal(match, want["match"]), what
    assert np.array_equal(sq.view(np.uint32), want["d2"].view(np.uint32)), what
    assert got["n_corr"] == want["n_corr"], what
    assert abs(got["mse"] - want["mse"]) <= 1e-12 * abs(want["mse"]), what
    assert np.linalg.norm(got["sums"] - want["sums"]) <= 1e-10 * np.linalg.norm(want["sums"]), what
    assert I.ulp_close(got["T_k"], want["T_k"]), (what, got["T_k"], want["T_k"])
    assert np.array_equal(g.working_cloud().view(np.uint32), W.view(np.uint32)), what
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("n", (1, 2, 3, 63, 64, 65, 255, 256, 257, 2048))
def test_estimate_sizes_poses_orders_inputs(reg, icp, odo, n):
    src, tgt, _, _, poses = odo
    for device_input in (False, True):
        for linear in (False, True):
            g = make(icp, reg, src[:n], tgt, device_input, linear)
            for k, T in enumerate(poses):
                want = check_estimate(g, src[:n], tgt, T, linear, False, (n, device_input, linear, k))
                assert want["estimated"] == (want["n_corr"] >= 3)
            g.close()


@pytest.mark.gpu
def test_estimate_multi_block_reduction(reg, icp, scene):
    src, tgt, _, guess = scene.make_pair(8192, 8192, scene.pair_seed(71, 0), "odometry")
    g = make(icp, reg, src, tgt)
    for recip in (False, True):
        g.setUseReciprocalCorrespondences(recip)
        want = check_estimate(g, src, tgt, guess, False, recip, recip)
        assert want["n_corr"] > 2000
    g.close()


@pytest.mark.gpu
def test_estimate_large_target(reg, icp, scene):
    """A target past the single-block sort (the regimes of tests/test_query_paths.py)."""
    src, tgt, _, guess = scene.make_pair(1025, 16385, scene.pair_seed(61, 0), "odometry")
    for device_input in (False, True):
        g = make(icp, reg, src, tgt, device_input)
        for recip in (False, True):
            g.setUseReciprocalCorrespondences(recip)
            check_estimate(g, src, tgt, guess, False, recip, (device_input, recip))
        g.close()


@pytest.mark.gpu
def test_reciprocal(reg, icp, odo, monkeypatch):
    src, tgt, _, guess, _ = odo
    g = make(icp, reg, src, tgt)
    fwd = check_estimate(g, src, tgt, guess, False, False, "forward")
    g.setUseReciprocalCorrespondences(True)
    rec = check_estimate(g, src, tgt, guess, False, True, "reciprocal")
    assert rec["n_corr"] < 0.6 * fwd["n_corr"] and rec["n_corr"] > 300, (fwd["n_corr"], rec["n_corr"])
    kept = rec["match"] >= 0
    assert np.array_equal(rec["match"][kept], fwd["match"][kept]) and np.array_equal(rec["d2"].view(np.uint32), fwd["d2"].view(np.uint32))
    got = (g.estimate(guess), *g.correspondences())
    # duplicated source points that share a nearest target: only the lowest index survives
    dup = np.concatenate([src[:300], src[:300], src[300:500]])
    set_clouds(g, dup, tgt)
    w = check_estimate(g, dup, tgt, guess, False, True, "duplicated source")
    assert np.all(w["match"][300:600] == -1) and np.count_nonzero(w["match"][:300] >= 0) > 50
    # duplicated target points: the forward tie goes to the lowest target index
    tdup = np.concatenate([tgt[:700], tgt[:700], tgt[700:]])
    set_clouds(g, src, tdup)
    for recip in (False, True):
        g.setUseReciprocalCorrespondences(recip)
        w = check_estimate(g, src, tdup, guess, False, recip, "duplicated target")
        assert not np.any((w["match"] >= 700) & (w["match"] < 1400))
    g.close()
    # the brute-force switch: the same bytes
    monkeypatch.setenv("APDGICP_ICP_RECIP_MODE", "brute")
    b = make(icp, reg, src, tgt)
    b.setUseReciprocalCorrespondences(True)
    e = b.estimate(guess)
    m, s = b.correspondences()
    assert np.array_equal(m, got[1]) and np.array_equal(s.view(np.uint32), got[2].view(np.uint32))
    assert e["T_k"].tobytes() == got[0]["T_k"].tobytes() and e["sums"].tobytes() == got[0]["sums"].tobytes() and e["mse"] == got[0]["mse"]
    check_estimate(b, src, tgt, guess, False, True, "brute")
    b.close()


@pytest.mark.gpu
def test_gate_at_the_exact_threshold(reg, icp):
    """max_correspondence_distance = 2.5, whose square is exact: d2 = 6.25 is kept, nextafter(6.25) is rejected, in both directions."""
    dy = f32(np.sqrt(np.spacing(f32(6.25))))
    above = f32(f32(2.5) * f32(2.5)) + dy * dy
    assert above == np.nextafter(f32(6.25), f32(np.inf))
    # (far apart and in general position: every coordinate and every offset below is exact in fp32)
    src = np.array([[0, 0, 0], [200, 0, 100], [0, 300, 200], [100, 100, 300], [300, 200, 400], [200, 300, 500]], dtype=f32)
    off = np.array([[2.5, 0, 0], [2.5, dy, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0]], dtype=f32)
    tgt = src + off
    for recip in (False, True):
        g = make(icp, reg, src, tgt)
        g.setUseReciprocalCorrespondences(recip)
        check_estimate(g, src, tgt, np.eye(4, dtype=f32), False, recip, recip)
        match, sq = g.correspondences()
        assert match.tolist() == [0, -1, 2, 3, 4, 5] and sq[0] == f32(6.25) and sq[1] == above
        g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("recip,linear", ((False, False), (True, False), (False, True)))
def test_trace_teacher_forced(reg, icp, odo, recip, linear):
    """Every iteration k re-run by the restatement from the device's own T_1 .. T_(k-1)."""
    src, tgt, _, guess, _ = odo
    src, tgt = src[:700], tgt[:900]
    g = make(icp, reg, src, tgt, linear=linear, transformation_epsilon=1e-12)
    g.setUseReciprocalCorrespondences(recip)
    g.setTransformationRotationEpsilon(2.0)   # (the transform test can never hold: the run goes on to max_iterations)
    for K in (1, 2, 3, 5):
        g.setMaximumIterations(K)
        T = g.align(guess)
        tr = g.trace()
        assert len(tr["n_corr"]) == K == g.nr_iterations and g.convergence_state() == icp.ITERATIONS and g.hasConverged()
        want = I.align(src, tgt, guess, max_iterations=K, transformation_epsilon=1e-12, max_dist=GATE, reciprocal=recip, rotation_epsilon=2.0, linear=linear,
                       forced_T=list(tr["T_k"]))
        assert np.array_equal(g.working_cloud().view(np.uint32), want["W"].view(np.uint32))
        assert T.tobytes() == want["T"].tobytes()      # IC6: the fp32 product of the trace
        for k, it in enumerate(want["trace"]):
            assert tr["n_corr"][k] == it["n_corr"]
            assert abs(tr["mse"][k] - it["mse"]) <= 1e-12 * it["mse"]
            assert I.ulp_close(tr["T_k"][k], it["T_k"]), (K, k)
        match, sq = g.correspondences()
        last = want["trace"][-1]
        assert np.array_equal(match, last["match"]) and np.array_equal(sq.view(np.uint32), last["d2"].view(np.uint32))
        assert g.result.n_matched == last["n_corr"] and g.result.final_cost == tr["mse"][-1]
        assert (g.result.n_linearize, g.result.n_compute_error, g.result.lm_failed) == (K, 0, 0)
    g.close()


@pytest.mark.gpu
def test_every_convergence_state(reg, icp, odo, scene):
    src, tgt, _, guess, _ = odo
    src, tgt = src[:800], tgt[:1000]
    g = make(icp, reg, src, tgt, transformation_epsilon=0.01)        # the factory's epsilon: t2 <= 0.01 is 0.1 m
    g.align(guess)
    assert (g.convergence_state(), g.nr_iterations, g.hasConverged()) == (icp.TRANSFORM, 1, True)
    g.setMaximumIterationsSimilarTransforms(2)                       # three consecutive similar iterations
    g.align(guess)
    assert (g.convergence_state(), g.nr_iterations, g.hasConverged()) == (icp.TRANSFORM, 3, True)
    assert g.trace()["similar"].tolist() == [1, 2, 2]
    g.setMaximumIterationsSimilarTransforms(0)
    g.setTransformationEpsilon(1e-8)
    g.setMaximumIterations(5)
    g.align(guess)
    assert (g.convergence_state(), g.nr_iterations, g.hasConverged()) == (icp.ITERATIONS, 5, True)
    g.setMaximumIterations(50)
    g.setTransformationRotationEpsilon(2.0)                          # the transform test can never hold
    g.setEuclideanFitnessEpsilon(0.5)
    g.align(guess)
    assert (g.convergence_state(), g.hasConverged()) == (icp.REL_MSE, True) and g.nr_iterations == 2
    g.setEuclideanFitnessEpsilon(-DBL_MAX)
    s2, t2, _ = rigid_copy(scene, 400, 9)
    set_clouds(g, s2, t2)
    g.align()
    assert (g.convergence_state(), g.hasConverged()) == (icp.ABS_MSE, True) and 2 <= g.nr_iterations < 50
    g.close()
    # NO_CORRESPONDENCES with 2 matches, against 3 matches running
    s3 = np.array([[0, 0, 0], [0, 0, 100], [0, 50, 200]], dtype=f32)
    for third, want_state in ((3.0, icp.NO_CORRESPONDENCES), (2.0, icp.TRANSFORM)):
        t3 = s3 + np.array([[0.5, 0, 0], [0.5, 0, 0], [third, 0, 0]], dtype=f32)
        h = make(icp, reg, s3, t3, transformation_epsilon=0.5, max_iterations=4)
        gs = scene.make_transform([0.01, 0, 0]).astype(f32)
        T = h.align(gs)
        assert h.convergence_state() == want_state and h.result.n_matched == (2 if third == 3.0 else 3)
        if want_state == icp.NO_CORRESPONDENCES:
            assert not h.hasConverged() and h.nr_iterations == 0 and T.tobytes() == gs.tobytes()
        else:
            assert h.hasConverged() and h.nr_iterations >= 1
        h.close()


FREE_RUNS = ((512, 640, 72, 0, False, 0.0), (512, 640, 72, 1, True, 0.0), (700, 600, 72, 2, False, 1e-6))


def free_run_reference(scene, case):
    ns, nt, cfg, k, recip, eps = case
    src, tgt, _, guess = scene.make_pair(ns, nt, scene.pair_seed(cfg, k), "odometry")
    kw = dict(max_iterations=10, transformation_epsilon=eps, max_dist=GATE, reciprocal=recip)
    return src, tgt, guess, kw, I.align(src, tgt, guess, want_second=True, **kw)


@pytest.mark.parametrize("case", FREE_RUNS)
def test_free_run_fixtures_have_a_margin(scene, case):
    """CPU: the restatement alone shows the margin the GPU comparison relies on."""
    *_, want = free_run_reference(scene, case)
    assert min(want["margins"]) > 1e-3 and want["min_gap_ulps"] > 4 and want["iterations"] >= 2


@pytest.mark.gpu
@pytest.mark.parametrize("case", FREE_RUNS)
def test_free_run_against_the_restatement(reg, icp, scene, case):
    src, tgt, guess, kw, want = free_run_reference(scene, case)
    assert min(want["margins"]) > 1e-3 and want["min_gap_ulps"] > 4
    g = make(icp, reg, src, tgt, transformation_epsilon=kw["transformation_epsilon"], max_iterations=kw["max_iterations"])
    g.setUseReciprocalCorrespondences(kw["reciprocal"])
    T = g.align(guess)
    assert (g.convergence_state(), g.nr_iterations, g.result.n_matched, g.hasConverged()) == (want["state"], want["iterations"], want["n_matched"], want["converged"])
    te, re_ = scene.pose_error(want["T"], T)
    assert te <= 1e-3 and re_ <= 1e-4
    g.close()


@pytest.mark.gpu
def test_mode_rules(reg, icp, odo, scene):
    src, tgt, _, guess, _ = odo
    src, tgt = src[:600], tgt[:800]
    L = reg.load_library()
    live0 = (ctypes.c_int64(), ctypes.c_int64())
    L.apdgicp_debug_live_buffers(ctypes.byref(live0[0]), ctypes.byref(live0[1]))
    vg = importlib.import_module("riv-slam_amd.vgicp")
    nd = importlib.import_module("riv-slam_amd.ndt")
    kw = dict(max_correspondence_distance=2.0, transformation_epsilon=0.01)
    fresh = reg.FastAPDGICP(reg.default_params(**kw), device=0)
    set_clouds(fresh, src, tgt)
    T_apd = fresh.align(guess)
    rec_apd = bytes(fresh.result)
    fresh.close()
    g = icp.ICP(reg.default_params(**kw), device=0)
    set_clouds(g, src, tgt)
    assert g.enabled()
    # exclusivity with voxelized GICP and NDT
    on = ctypes.c_int()
    L.apdgicp_set_vgicp(g.h, ctypes.byref(vg.default_vgicp_params()))
    assert not g.enabled() and L.apdgicp_get_vgicp(g.h, None, ctypes.byref(on)) == 0 and on.value == 1
    g.enable()
    assert g.enabled() and L.apdgicp_get_vgicp(g.h, None, ctypes.byref(on)) == 0 and on.value == 0
    L.apdgicp_set_ndt(g.h, ctypes.byref(nd.default_ndt_params()))
    assert not g.enabled() and L.apdgicp_get_ndt(g.h, None, ctypes.byref(on)) == 0 and on.value == 1
    g.enable()
    assert g.enabled() and L.apdgicp_get_ndt(g.h, None, ctypes.byref(on)) == 0 and on.value == 0
    # the unsupported calls
    for call in (lambda: g.linearize(np.eye(4)), lambda: g.compute_error(np.eye(4)), g.getFinalHessian, lambda: reg.FastAPDGICP.correspondences(g), g.mahalanobis):
        with pytest.raises(reg.ApdgicpError) as ei:
            call()
        assert ei.value.code == -5
    with pytest.raises(reg.ApdgicpError) as ei:
        g.correspondences()          # nothing estimated yet
    assert ei.value.code == -3
    # an ICP align, then the queries that keep working
    T = g.align(guess)
    assert g.hasConverged() and g.convergence_state() == icp.TRANSFORM
    idx, sqd = g.nearestNeighbours(T)
    Wt = I.transform(T, src)
    wi, wd = I.nearest(Wt, tgt)
    assert np.array_equal(idx, wi) and np.array_equal(sqd.view(np.uint32), wd.view(np.uint32))
    # (apdgicp_transform_source is pcl::transformPointCloud's left-to-right sum whatever the handle's order, as tests/test_query_paths.py pins it)
    assert np.array_equal(g.transformSource(T).view(np.uint32), I.transform(T, src, linear=True).view(np.uint32))
    score = g.getFitnessScore(4.0, T)
    inl = wd.astype(np.float64)[wd <= 4.0]
    assert g.last_inliers == len(inl) and abs(score - inl.mean()) <= 1e-9 * inl.mean()
    assert 0.0 < g.inlierFraction(0.5, T) <= 1.0
    qi, _ = g.nearestNeighboursOf(tgt[:10] + f32(1e-3))
    assert np.array_equal(qi, np.arange(10))
    g.correspondences()   # (still those of the align: the queries left them alone)
    # with the mode off: the bytes of a fresh APD handle
    g.disable()
    assert not g.enabled()
    assert g.align(guess).tobytes() == T_apd.tobytes() and bytes(g.result) == rec_apd
    with pytest.raises(reg.ApdgicpError):
        g.estimate(guess)
    # a 5-point cloud aligns although k = 20; a reused handle with changed clouds and parameters
    g.enable()
    s5, t5, T5 = rigid_copy(scene, 5, 12)
    set_clouds(g, s5, t5)
    g.setMaxCorrespondenceDistance(1.0)
    g.setTransformationEpsilon(1e-10)
    g.setMaximumIterations(3)
    T = g.align()
    assert g.result.n_matched == 5 and np.abs(T.astype(np.float64) - T5).max() <= 1e-5
    want = I.align(s5, t5, None, max_iterations=3, transformation_epsilon=1e-10, max_dist=1.0)
    assert (g.convergence_state(), g.nr_iterations) == (want["state"], want["iterations"])
    g.setUseReciprocalCorrespondences(True)
    g.setMaxCorrespondenceDistance(GATE)
    set_clouds(g, src[:333], tgt)
    check_estimate(g, src[:333], tgt, guess, False, True, "reused")
    g.swapSourceAndTarget()
    with pytest.raises(reg.ApdgicpError):
        g.working_cloud()            # the estimate described the other clouds
    assert (g.n_src, g.n_tgt) == (len(tgt), 333)
    check_estimate(g, tgt, src[:333], np.linalg.inv(guess.astype(np.float64)).astype(f32), False, True, "swapped")
    g.clearSource()
    with pytest.raises(reg.ApdgicpError) as ei:
        g.align(guess)
    assert ei.value.code == -3
    g.close()
    live1 = (ctypes.c_int64(), ctypes.c_int64())
    L.apdgicp_debug_live_buffers(ctypes.byref(live1[0]), ctypes.byref(live1[1]))
    assert (live1[0].value, live1[1].value) == (live0[0].value, live0[1].value)


@pytest.mark.gpu
@pytest.mark.parametrize("recip", (False, True))
def test_determinism(reg, icp, odo, recip):
    src, tgt, _, guess, _ = odo
    runs = []
    for _ in range(2):
        g = make(icp, reg, src, tgt, transformation_epsilon=1e-9, max_iterations=6)
        g.setUseReciprocalCorrespondences(recip)
        g.align(guess)
        tr = g.trace()
        m, s = g.correspondences()
        runs.append((bytes(g.result), tr["T_k"].tobytes(), tr["n_corr"].tobytes(), tr["mse"].tobytes(), tr["similar"].tobytes(), g.working_cloud().tobytes(),
                     m.tobytes(), s.tobytes(), g.estimate(guess)["sums"].tobytes()))
        g.close()
    assert runs[0] == runs[1]
