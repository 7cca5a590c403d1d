"""Voxelized GICP as a mode of the BATCH handle: include/apdgicp_hip.h V8 .. V12, riv-slam_amd/csrc/apd_vgicp_batch.hpp,
riv-slam_amd/vgicp.py (BatchVGICP), against the single handle (tests/test_vgicp.py checks that one against the restatement) and the
restatement tests/vgicp_np.py itself.

CPU part: exports, the Python class, the argument checks that need no handle, and the face margin of every align fixture used below.
GPU part (-m gpu): maps bit for bit, the first linearize bit for bit, align parity, composition independence, V7 inside a batch, the
cache rules, an invalid target, the calls the mode does not offer, and loop verification through loop_verifier.verify_candidates.

Bars.  Maps, the first linearize and everything compared batch against batch: bytes.  Align against the single handle: the integer
fields equal, final_cost 1e-11 relative (the project's TRACE_TOL), every element of T within one float ulp; against the restatement
1e-3 m / 1e-4 rad.  The integer fields can be exact because sin / cos of the step (device library here, the host's there) move an
iterate in its last bits only and every align fixture keeps its transformed points >= 1e-9 voxel edges from a voxel face over the
whole run -- asserted on the CPU for each fixture (test_align_fixtures_keep_their_distance_from_the_voxel_faces) and again for the
run the GPU test makes.

How the six ALIGN_CASES become batches: a batch handle has ONE set of parameters, one search method and one resolution, so the six
tuples cannot share a batch.  Each tuple (x LM, GN) is one batch of six pairs instead: the tuple's own fixture
scene.make_pair(2048, 4099, scene.pair_seed(7, idx)) and five variants of it against the same target -- the first
2048 / 1024 / 513 / 257 / 129 / 65 source points, each from its own perturbed guess -- so that pairs of different sizes finish after
different numbers of iterations and idle beside running ones.

The parameter round trip through apdgicp_batch_get_vgicp needs a handle, and a handle needs a device: it is in the GPU part
(test_params_round_trip_and_multiplicative_is_refused); the CPU part checks the refusal through the argument checks alone.
"""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest

import apdgicp_np as anp
import vgicp_np as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACE_TOL = 1e-11
FACE_MARGIN = 1e-9
LAUNCH = dict(max_correspondence_distance=2.0, transformation_epsilon=0.1)
NEW_SYMBOLS = ("apdgicp_batch_set_vgicp", "apdgicp_batch_get_vgicp", "apdgicp_batch_vgicp_voxel_count", "apdgicp_batch_vgicp_get_voxels",
               "apdgicp_batch_vgicp_build_count")
# (name, parameters, search, resolution, pair seed index): the tuples of tests/test_vgicp.py
ALIGN_CASES = (
    ("launch_d1", LAUNCH, 0, 1.0, 0),
    ("launch_d7", LAUNCH, 1, 1.0, 1),
    ("default_d1", {}, 0, 1.0, 2),
    ("default_d7", {}, 1, 1.0, 7),
    ("plane_d7_res2", dict(regularization=3, transformation_epsilon=0.01), 1, 2.0, 4),
    ("frobenius_d1", dict(regularization=4, transformation_epsilon=0.01), 0, 1.0, 5),
)
VARIANT_SIZES = (2048, 1024, 513, 257, 129, 65)
INT_FIELDS = ("converged", "iterations", "n_linearize", "n_compute_error", "lm_failed", "n_matched")


@pytest.fixture(scope="module")
def reg():
    import __graft_entry__ as g
    g.build()
    return importlib.import_module("riv-slam_amd.registration")


@pytest.fixture(scope="module")
def vg(reg):
    return importlib.import_module("riv-slam_amd.vgicp")


def _case_pairs(scene, name):
    """The six pairs of one tuple's batch: (parameters, search, resolution, target, [(source, guess)])."""
    tag, kw, search, res, idx = next(c for c in ALIGN_CASES if c[0] == name)
    src, tgt, _, guess = scene.make_pair(2048, 4099, scene.pair_seed(7, idx), "odometry")
    pairs = []
    for k, n in enumerate(VARIANT_SIZES):
        P = scene.make_transform(np.array([0.04 * k, -0.03 * k, 0.01 * k]), 0.003 * k, 0.0, 0.0)
        pairs.append((src[:n], (P @ guess.astype(np.float64)).astype(np.float32)))
    return kw, search, res, tgt, pairs


# ====================================================================== CPU
def test_new_symbols_are_exported_and_the_class_imports(reg, vg):
    L = reg.load_library()
    header = open(os.path.join(ROOT, "include", "apdgicp_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), f"{name} is not exported"
        assert name in reg.SYMBOLS
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared"
    assert "Batch handles have no such mode" not in header
    for v in ("V8.", "V9.", "V10.", "V11.", "V12."):
        assert v in header
    assert issubclass(vg.BatchVGICP, reg.BatchAPDGICP)
    for m in ("setResolution", "setNeighborSearchMethod", "setVoxelAccumulationMode", "enable", "disable", "enabled", "voxel_count", "voxels", "build_count",
              "get_vgicp", "align", "align_async", "synchronize", "fitness", "set_clouds"):
        assert callable(getattr(vg.BatchVGICP, m))
    assert L.apdgicp_abi_version() == 6


def test_set_vgicp_checks_its_parameters_before_anything_else(reg, vg):
    """The parameter checks need no handle: MULTIPLICATIVE is refused as UNSUPPORTED (V7), a resolution that is not positive and an
    unknown search method as INVALID_ARG; valid parameters reach the handle check (INVALID_ARG: the handle is null)."""
    L = reg.load_library()
    p = vg.default_vgicp_params()
    assert L.apdgicp_batch_set_vgicp(None, ctypes.byref(p)) == -1
    p.voxel_mode = vg.MULTIPLICATIVE
    assert L.apdgicp_batch_set_vgicp(None, ctypes.byref(p)) == -5
    p = vg.default_vgicp_params()
    p.resolution = 0.0
    assert L.apdgicp_batch_set_vgicp(None, ctypes.byref(p)) == -1
    p = vg.default_vgicp_params()
    p.neighbor_search = 3
    assert L.apdgicp_batch_set_vgicp(None, ctypes.byref(p)) == -1
    n = ctypes.c_int64()
    assert L.apdgicp_batch_vgicp_build_count(None, ctypes.byref(n)) == -1
    assert L.apdgicp_batch_get_vgicp(None, None, None) == -1


@pytest.mark.parametrize("name", [c[0] for c in ALIGN_CASES])
def test_align_fixtures_keep_their_distance_from_the_voxel_faces(scene, name):
    """The condition under which integer fields can be compared exactly, with the restatement alone (its own covariances), LM and GN,
    for every pair of every batch of test_align_parity -- the smaller variants included."""
    kw, search, res, tgt, pairs = _case_pairs(scene, name)
    p = anp.Params(**kw)
    tcov = anp.calculate_covariances(tgt, p.k_correspondences, p.regularization)
    iterations = set()
    for src, guess in pairs:
        scov = anp.calculate_covariances(src, p.k_correspondences, p.regularization)
        for optimizer in (0, 1):
            o = V.FastVGICP(anp.Params(**dict(kw, optimizer=optimizer)), resolution=res, search=search)
            o.setInputSource(src)
            o.setInputTarget(tgt)
            o.source_covs, o.target_covs = scov, tcov
            o.align(guess)
            assert o.face_margin_min >= FACE_MARGIN, (len(src), optimizer, o.face_margin_min)
            assert o.n_matched > len(src) // 4 and o.converged
            iterations.add(o.nr_iterations)
    assert len(iterations) >= 2   # the pairs of a batch do not all finish in the same tick


# ====================================================================== GPU
gpu = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _covs3(c):
    return np.ascontiguousarray(c[:, :3, :3])


def _assert_map_equal(got, want):
    assert np.array_equal(got["coords"], want["coords"])
    assert np.array_equal(got["counts"], want["counts"])
    assert np.array_equal(_bits(got["means"]), _bits(want["means"]))
    assert np.array_equal(_bits(got["covs"]), _bits(want["covs"]))


def _scene_cloud(n, seed=21):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(n, 3)) * [7, 7, 1.5]).astype(np.float32)


def _T(rec):
    return np.asarray(rec["T"], dtype=np.float32).reshape(4, 4).T


def _batch(reg, vg, search=0, res=1.0, **kw):
    b = vg.BatchVGICP(reg.default_params(**kw))
    b.setResolution(res)
    b.setNeighborSearchMethod(search)
    return b


def _single(reg, vg, src, tgt, search=0, res=1.0, **kw):
    g = vg.FastVGICP(reg.default_params(**kw))
    g.setResolution(res)
    g.setNeighborSearchMethod(search)
    g.setInputSource(src)
    g.setInputTarget(tgt)
    return g


@gpu
def test_params_round_trip_and_multiplicative_is_refused(reg, vg):
    b = vg.BatchVGICP()
    p, on = b.get_vgicp()
    assert on and b.enabled() and (p.resolution, p.neighbor_search, p.voxel_mode) == (1.0, vg.DIRECT1, vg.ADDITIVE)
    b.setResolution(0.75)
    b.setNeighborSearchMethod(vg.DIRECT27)
    b.setVoxelAccumulationMode(vg.ADDITIVE_WEIGHTED)
    p, on = b.get_vgicp()
    assert on and (p.resolution, p.neighbor_search, p.voxel_mode) == (0.75, vg.DIRECT27, vg.ADDITIVE_WEIGHTED)
    with pytest.raises(reg.ApdgicpError) as ei:
        b.setVoxelAccumulationMode(vg.MULTIPLICATIVE)
    assert ei.value.code == -5
    p, on = b.get_vgicp()
    assert on and (p.resolution, p.neighbor_search, p.voxel_mode) == (0.75, vg.DIRECT27, vg.ADDITIVE_WEIGHTED) and b.vparams.voxel_mode == vg.ADDITIVE_WEIGHTED
    b.disable()
    assert not b.enabled() and b.get_vgicp()[0].resolution == 0.75
    with pytest.raises(reg.ApdgicpError) as ei:
        b.voxel_count(0)
    assert ei.value.code == -3
    b.enable()
    assert b.enabled()
    assert b.L.apdgicp_batch_is_pooled(b.b) == 0
    b.set_pair_groups(2)   # accepted, no effect


# ---------------------------------------------------------------------- 1. maps (V8)
@gpu
def test_maps_bit_for_bit_and_one_build_per_distinct_target(reg, vg):
    sizes = (20, 63, 64, 65, 257, 4099)
    clouds = [_scene_cloud(n) for n in sizes]
    extra = _scene_cloud(300, 5)
    b = _batch(reg, vg)
    b.set_clouds(0, clouds + [extra])
    # every cloud of `sizes` is a target; slot 4 (257 points) is also the source of the pair against slot 5; slot 6 is a source only
    pairs = [(6, t) for t in range(6)] + [(4, 5)]
    assert b.build_count() == 0
    b.align(pairs)
    assert b.build_count() == 6
    for t, cloud in enumerate(clouds):
        g = vg.FastVGICP()
        g.setInputTarget(cloud)
        _assert_map_equal(b.voxels(t), g.voxels())
        assert b.voxel_count(t) == g.voxel_count()
    assert b.build_count() == 6                    # the getters found every map there
    assert b.voxel_count(6) > 0 and b.build_count() == 7   # a source-only slot had none until it was asked for


# ---------------------------------------------------------------------- 2. first linearize (V9)
@gpu
@pytest.mark.parametrize("search", (0, 1, 2))
def test_first_linearize_bit_for_bit(reg, vg, scene, search):
    sizes = (20, 64, 65, 257, 2048)
    src, tgt, _, guess = scene.make_pair(2048, 4099, scene.pair_seed(7, 0), "odometry")
    b = _batch(reg, vg, search, optimizer=1, max_iterations=1)
    b.set_clouds(0, [tgt] + [src[:n] for n in sizes])
    recs = b.align([(1 + i, 0) for i in range(len(sizes))], [guess] * len(sizes))   # grid x is sized by the 2048-point pair
    for i, n in enumerate(sizes):
        g = _single(reg, vg, src[:n], tgt, search)
        cost, _, _ = g.linearize(guess.astype(np.float64))
        matched = int((g.voxel_correspondences() >= 0).sum())
        assert matched > 0
        assert np.float64(recs[i]["final_cost"]).view(np.uint64) == np.float64(cost).view(np.uint64), (n, recs[i]["final_cost"], cost)
        assert int(recs[i]["n_matched"]) == matched
        assert (int(recs[i]["n_linearize"]), int(recs[i]["n_compute_error"]), int(recs[i]["iterations"])) == (1, 0, 0)


# ---------------------------------------------------------------------- 3. align parity (V10)
@gpu
@pytest.mark.parametrize("optimizer", (0, 1), ids=("lm", "gn"))
@pytest.mark.parametrize("name", [c[0] for c in ALIGN_CASES])
def test_align_parity(reg, vg, scene, name, optimizer):
    kw, search, res, tgt, pairs = _case_pairs(scene, name)
    kw = dict(kw, optimizer=optimizer)
    b = _batch(reg, vg, search, res, **kw)
    b.set_clouds(0, [tgt] + [s for s, _ in pairs])
    recs = b.align([(1 + i, 0) for i in range(len(pairs))], [g for _, g in pairs])
    ticks = b.last_ticks()[0]
    seen = set()
    for i, (src, guess) in enumerate(pairs):
        g = _single(reg, vg, src, tgt, search, res, **kw)
        T = g.align(guess)
        r, w = recs[i], g.result
        got = tuple(int(r[k]) for k in INT_FIELDS)
        want = (int(w.converged), w.iterations, w.n_linearize, w.n_compute_error, w.lm_failed, w.n_matched)
        rel = abs(float(r["final_cost"]) - w.final_cost) / w.final_cost
        ulps = np.abs(_T(r).astype(np.float64) - T.astype(np.float64)) / np.spacing(np.maximum(np.abs(_T(r)), np.abs(T.astype(np.float32))))
        # the restatement with the device's covariances: the margin of this very run, and the pose
        o = V.FastVGICP(anp.Params(**kw), resolution=res, search=search)
        o.setInputSource(g.getPoints(0))
        o.setInputTarget(g.getPoints(1))
        o.source_covs, o.target_covs = _covs3(g.getSourceCovariances()), _covs3(g.getTargetCovariances())
        To = o.align(guess)
        te, re_ = scene.pose_error(To, _T(r))
        print(name, "lm" if optimizer == 0 else "gn", len(src), "record", got, "cost rel", rel, "T ulps", ulps.max(), "pose", te, re_, "face margin", o.face_margin_min)
        assert o.face_margin_min >= FACE_MARGIN
        assert got == want, (len(src), got, want)
        assert got == (int(o.converged), o.nr_iterations, o.trace.n_linearize, o.trace.n_compute_error, 0, o.n_matched)
        assert rel <= TRACE_TOL
        assert ulps.max() <= 1.0
        assert te <= 1e-3 and re_ <= 1e-4
        seen.add((got[2], got[3]))
    assert len(seen) >= 2                      # pairs finished in different ticks
    assert ticks >= max(a + c for a, c in seen)


# ---------------------------------------------------------------------- 4. composition independence (V11)
@gpu
def test_a_record_is_a_pure_function_of_the_pair(reg, vg, scene):
    sizes = (20, 64, 65, 257, 1024, 2048)
    srcA, tgtA, _, gA = scene.make_pair(2048, 4099, scene.pair_seed(7, 0), "odometry")
    srcB, tgtB, _, gB = scene.make_pair(2048, 4099, scene.pair_seed(7, 1), "odometry")
    b = _batch(reg, vg, vg.DIRECT7)
    b.set_clouds(0, [tgtA, tgtB] + [srcA[:n] for n in sizes] + [srcB[:n] for n in sizes])
    pairs = [(2 + i, 0) for i in range(6)] + [(8 + i, 1) for i in range(6)]
    pairs = [pairs[i] for i in (0, 6, 1, 7, 2, 8, 3, 9, 4, 10, 5, 11)]   # the two targets interleaved
    guesses = [gA if t == 0 else gB for _, t in pairs]
    whole = b.align(pairs, guesses)
    assert sum(int(r["converged"]) for r in whole) >= 10 and len({int(r["n_linearize"]) for r in whole}) >= 2
    rev = b.align(pairs[::-1], guesses[::-1])[::-1]
    again = b.align(pairs, guesses)
    for i in range(12):
        alone = b.align([pairs[i]], [guesses[i]])[0]
        assert whole[i].tobytes() == rev[i].tobytes() == again[i].tobytes() == alone.tobytes(), i
    fresh = _batch(reg, vg, vg.DIRECT7)
    fresh.set_clouds(0, [tgtB, srcB[:257]])
    i = pairs.index((2 + 6 + 3, 1))
    assert fresh.align([(1, 0)], [gB])[0].tobytes() == whole[i].tobytes()   # a first align on another handle, other slots


# ---------------------------------------------------------------------- 5. V7 inside a batch
@gpu
@pytest.mark.parametrize("optimizer", (0, 1), ids=("lm", "gn"))
def test_a_pair_without_correspondences_ends_alone(reg, vg, scene, optimizer):
    src, tgt, _, guess = scene.make_pair(2048, 4099, scene.pair_seed(7, 0), "odometry")
    far = src[:257] + np.float32(5000.0)
    g_far = np.eye(4, dtype=np.float32)
    g_far[:3, 3] = (0.5, 0.25, -0.125)
    b = _batch(reg, vg, vg.DIRECT27, optimizer=optimizer)
    b.set_clouds(0, [tgt, src, far, src[:513]])
    with_far = b.align([(1, 0), (2, 0), (3, 0)], [guess, g_far, guess])
    r = with_far[1]
    assert tuple(int(r[k]) for k in INT_FIELDS) == (0, 0, 1, 0, 0, 0)
    assert np.array_equal(_T(r), g_far) and float(r["final_cost"]) == 0.0
    without = b.align([(1, 0), (3, 0)], [guess, guess])
    assert with_far[0].tobytes() == without[0].tobytes() and with_far[2].tobytes() == without[1].tobytes()
    assert int(without[0]["converged"]) == 1 and int(without[0]["n_matched"]) > 500


# ---------------------------------------------------------------------- 6. cache rules
@gpu
def test_cache_rules_and_the_apd_path_is_left_alone(reg, vg, scene):
    srcA, tgtA, _, gA = scene.make_pair(2048, 4099, scene.pair_seed(7, 0), "odometry")
    srcB, tgtB, _, gB = scene.make_pair(2048, 4099, scene.pair_seed(7, 1), "odometry")
    b = _batch(reg, vg)
    b.set_clouds(0, [tgtA, tgtB, srcA, srcB])
    pairs, guesses = [(2, 0), (3, 1), (2, 1)], [gA, gB, gA]     # three pairs, two distinct targets
    first = b.align(pairs, guesses)
    assert b.build_count() == 2
    assert b.align(pairs, guesses).tobytes() == first.tobytes() and b.build_count() == 2    # unchanged clouds: no build
    b.set_cloud(1, tgtB[:4000])
    b.align(pairs, guesses)
    assert b.build_count() == 3                                  # exactly the slot that was set again
    b.set_cloud(2, srcA[:1000])                                  # a source-only slot has no map
    b.align(pairs, guesses)
    assert b.build_count() == 3
    b.setNeighborSearchMethod(vg.DIRECT7)                        # the search method is no property of a map
    b.align(pairs, guesses)
    assert b.build_count() == 3
    b.setResolution(0.5)
    b.align(pairs[:1], guesses[:1])
    assert b.build_count() == 4                                  # another resolution: exactly the targets USED
    b.align(pairs, guesses)
    assert b.build_count() == 5
    b.disable()
    b.enable()
    b.align(pairs, guesses)
    assert b.build_count() == 5                                  # off and on, nothing else changed
    p = reg.default_params(k_correspondences=10)
    b.set_params(p)                                              # invalidates the covariances, hence the maps of the targets used
    b.align(pairs, guesses)
    assert b.build_count() == 7
    # mode off: an APD batch as on a handle that never had the mode on
    b.disable()
    apd = b.align(pairs, guesses)
    ref = reg.BatchAPDGICP(p)
    ref.set_clouds(0, [tgtA, tgtB[:4000], srcA[:1000], srcB])
    assert ref.align(pairs, guesses).tobytes() == apd.tobytes()
    assert b.build_count() == 7
    b.enable()
    b.clear()                                                    # apdgicp_batch_clear drops every map
    b.set_clouds(0, [tgtA, tgtB[:4000], srcA[:1000], srcB])
    b.align(pairs, guesses)
    assert b.build_count() == 9


# ---------------------------------------------------------------------- 7. invalid target
@gpu
def test_a_target_with_a_nan_point_fails_the_align_and_the_handle_stays_usable(reg, vg, scene):
    src, tgt, _, guess = scene.make_pair(2048, 4099, scene.pair_seed(7, 0), "odometry")
    bad = tgt[:700].copy()
    bad[5, 1] = np.nan
    b = _batch(reg, vg)
    b.set_clouds(0, [tgt, bad, src[:513]])
    ok = b.align([(2, 0)], [guess])
    with pytest.raises(reg.ApdgicpError) as ei:
        b.align([(2, 0), (2, 1)], [guess, guess])
    assert ei.value.code == -1 and "slot 1" in str(ei.value) and "point 5" in str(ei.value)
    b.set_cloud(1, tgt[:700])
    recs = b.align([(2, 0), (2, 1)], [guess, guess])
    assert recs[0].tobytes() == ok[0].tobytes() and int(recs[1]["n_linearize"]) >= 1


# ---------------------------------------------------------------------- 8. unsupported calls
@gpu
def test_enqueue_is_unsupported_with_the_mode_on(reg, vg, scene):
    src, tgt, _, guess = scene.make_pair(257, 700, scene.pair_seed(7, 0), "odometry")
    b = _batch(reg, vg, optimizer=1)
    b.set_clouds(0, [tgt, src])
    with pytest.raises(reg.ApdgicpError) as ei:
        b.align_enqueue([(1, 0)], [guess])
    assert ei.value.code == -5 and "apdgicp_batch_set_vgicp" in str(ei.value)
    assert b.L.apdgicp_batch_pump(b.b) == -5
    ptr, nbytes = b.align_async([(1, 0)], [guess])            # complete on return
    assert ptr and nbytes == 96
    out = np.zeros(1, dtype=reg.RESULT_DTYPE)
    b.copy_results_to(out, 1)
    b.synchronize()
    assert out.tobytes() == b.align([(1, 0)], [guess]).tobytes()
    b.disable()
    t = b.align_enqueue([(1, 0)], [guess])                    # the APD path offers it again
    assert len(b.align_collect(t)) == 1


# ---------------------------------------------------------------------- 9. consumers
@gpu
def test_verify_candidates_picks_what_a_loop_of_single_handles_picks(reg, vg, scene):
    lv = importlib.import_module("riv-slam_amd.loop_verifier")
    # the new keyframe (the scan) is the TARGET, the six keyframes before it are the candidates (loop_detector.cpp:392-411)
    tgt, cands, _, to_keyframe = scene.make_keyframe_set(4099, 2048, 6, scene.pair_seed(7, 3))
    guesses = [np.linalg.inv(g.astype(np.float64)).astype(np.float32) for g in to_keyframe]
    kw = dict(transformation_epsilon=0.1)
    b = _batch(reg, vg, vg.DIRECT7, **kw)
    thresh = 2.0   # (keyframes up to six odometry steps away see other parts of the street: the scores of this set are 0.8 .. 1.5 m^2)
    loop, scores, results = lv.verify_candidates(b, tgt, cands, guesses, fitness_score_thresh=thresh)
    best_score, best = np.finfo(np.float64).max, -1
    for i, (c, guess) in enumerate(zip(cands, guesses)):
        g = _single(reg, vg, c, tgt, vg.DIRECT7, **kw)
        T = g.align(guess)
        score = g.getFitnessScore()
        te, re_ = scene.pose_error(T, _T(results[i]))
        assert te <= 1e-3 and re_ <= 1e-4 and bool(results[i]["converged"]) == g.hasConverged()
        assert abs(scores[i] - score) <= 1e-3 * score
        if not g.hasConverged() or score > best_score:
            continue
        best_score, best = score, i
    print("scores", scores, "best", best)
    assert best >= 0 and best_score <= thresh and len(set(np.round(scores, 6))) == 6
    assert loop is not None and loop.candidate == best
    assert b.build_count() == 1
