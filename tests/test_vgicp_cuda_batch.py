"""FAST_VGICP_CUDA as a mode of the BATCH handle, on the GPU: include/apdgicp_hip.h VC11 .. VC16, riv-slam_amd/csrc/apd_vgicp_cuda_batch.hpp,
riv-slam_amd/vgicp_cuda.py (BatchVGICPCuda), against the single handle in this mode (tests/test_vgicp_cuda.py checks that one against the
restatement) and the restatement tests/vgicp_cuda_np.py itself.  (The part that needs no GPU: tests/test_vgicp_cuda_batch_cpu.py.)

Bars.  Prepared clouds, maps, the first linearize (cost, n_matched and the frozen indices; H and b of a pair's first linearize are not
readable from a batch handle, so they are compared through the cost and the indices only) and everything compared batch against batch:
bytes.  Align against the single handle: the integer fields equal for every pair; for the pairs that converge (vgicp_cuda_batch_cases.
CONVERGING, asserted on the CPU) final_cost 1e-11 relative and every element of T within one float ulp -- the bars of
tests/test_vgicp_batch.py, for the same reason: sin / cos of the step come from the device library here and from the host's there, which
moves an iterate in its last bits only, and every fixture keeps its transformed points >= 1e-9 voxel edges from a voxel face over the whole
run (asserted on the CPU for each batch and again here for the run the GPU made).  Against the restatement 1e-3 m / 1e-4 rad.  Kept lists
are exact because every cloud keeps > 1e-9 from the PLANE threshold (asserted on the CPU, and here against the restatement's lists).

Sizes: the block edges of the new kernels -- VC_K = 20, the wave 64, VG_BLK 256, VC_BLK / SCAN_BLK 1024 -- as prefixes of
tests/golden/vgicp_cuda_pair.npz."""
import importlib

import numpy as np
import pytest

import vgicp_cuda_batch_cases as K
import vgicp_cuda_np as VC

TRACE_TOL = 1e-11
INT_FIELDS = ("converged", "iterations", "n_linearize", "n_compute_error", "lm_failed", "n_matched")
gpu = pytest.mark.gpu


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
def guesses(pair):
    return K.batch_guesses(pair)


@pytest.fixture(scope="module")
def d1_whole(reg, vc, pair, guesses):
    """The records of the seven-pair DIRECT1 batch (three of its pairs do not converge), computed once and left unchanged: what the tests of
    VC15, of the degenerate pairs, of the refusals and of the cache rules compare their own runs with."""
    b = _batch(vc, reg)
    tgt, srcs = K.batch_clouds(pair)
    b.set_clouds(0, [tgt] + srcs)
    return b.align(_pairs(7), guesses)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _T(rec):
    return np.asarray(rec["T"], dtype=np.float32).reshape(4, 4).T


def _ints(rec):
    return tuple(int(rec[k]) for k in INT_FIELDS)


def _pairs(n, first=1, target=0):
    return [(first + i, target) for i in range(n)]


def _batch(vc, reg, search=0, radius=1.5, regularization=VC.PLANE, res=1.0, **kw):
    b = vc.BatchVGICPCuda(reg.default_params(**kw))
    b.setRegularizationMethod(regularization)
    b.setNeighborSearchMethod(search, radius)
    b.setResolution(res)
    return b


def _single(vc, reg, src, tgt, search=0, radius=1.5, regularization=VC.PLANE, res=1.0, **kw):
    g = vc.FastVGICPCuda(reg.default_params(**kw))
    g.setRegularizationMethod(regularization)
    g.setNeighborSearchMethod(search, radius)
    g.setResolution(res)
    if src is not None:
        g.setInputSource(src)
    if tgt is not None:
        g.setInputTarget(tgt)
    return g


def _assert_map_equal(got, want):
    assert np.array_equal(got["coords"], want["coords"])
    assert np.array_equal(got["counts"], want["counts"])
    assert np.array_equal(_bits(got["means"]), _bits(want["means"]))
    assert np.array_equal(_bits(got["covs"]), _bits(want["covs"]))


# ---------------------------------------------------------------------- 1. prepared slots (VC11)
@gpu
@pytest.mark.parametrize("method", (VC.PLANE, VC.MIN_EIG, VC.FROBENIUS), ids=("plane", "min_eig", "frobenius"))
def test_prepared_slots_bit_for_bit_and_one_wait_for_all(vc, reg, pair, method):
    clouds = [pair["target"][:n] for n in K.TARGET_PREFIXES]
    b = _batch(vc, reg, regularization=method, optimizer=1, max_iterations=1)
    b.set_clouds(0, clouds)
    assert b.build_count() == (0, 0) and b.debug_counts()[:2] == (0, 0)
    # one align names every slot: each is the source of one pair and slot 11 (2048 points) the target of all
    b.align([(i, 11) for i in range(12)])
    assert b.build_count() == (12, 1)
    assert b.debug_counts()[:2] == (1, 1)          # ONE host wait prepared the twelve slots, one more built the map
    g = _single(vc, reg, None, None, regularization=method)
    for i, n in enumerate(K.TARGET_PREFIXES):
        g.setInputTarget(clouds[i])
        kept, want = b.kept(i), g.kept(1)
        assert kept.dtype == np.int32 and np.array_equal(kept, want), (n, len(kept), len(want))
        assert np.array_equal(kept, VC.prepare(clouds[i], method)["kept_index"]), n
        raw, covs = b.covariances(i)
        raw1, covs1 = g.covariances(1)
        assert np.array_equal(_bits(raw), _bits(raw1)) and np.array_equal(_bits(covs), _bits(covs1)), n
        if method != VC.PLANE:
            assert len(kept) == n
    assert b.build_count() == (12, 1) and b.debug_counts()[:2] == (1, 1)       # the getters found every slot prepared
    if method == VC.PLANE:
        assert len(b.kept(11)) == K.KEPT_TARGET[2048] and len(b.kept(9)) == K.KEPT_TARGET[1024] and len(b.kept(0)) == 20


# ---------------------------------------------------------------------- 2. maps (VC12)
@gpu
def test_maps_bit_for_bit_and_one_build_per_distinct_target(vc, reg, pair):
    clouds = [pair["target"][:n] for n in K.TARGET_PREFIXES]
    b = _batch(vc, reg, optimizer=1, max_iterations=1)
    b.set_clouds(0, clouds + [pair["source"][:257]])
    targets = [K.TARGET_PREFIXES.index(n) for n in (21, 257, 2048)]
    b.align([(12, t) for t in targets] + [(12, targets[2]), (targets[1], targets[2])])     # five pairs, three distinct targets
    assert b.build_count() == (4, 3) and b.debug_counts()[:2] == (1, 1)
    g = _single(vc, reg, None, None)
    for t in targets:
        g.setInputTarget(clouds[t])
        _assert_map_equal(b.voxels(t), g.voxels())
        assert b.voxel_count(t) == g.voxel_count() > 0
    assert b.build_count() == (4, 3)                # the getters found every map there
    assert b.voxel_count(12) > 0 and b.build_count() == (4, 4)     # a source-only slot had none until it was asked for
    assert b.voxel_count(0) > 0 and b.build_count() == (5, 5)      # a slot no pair named: prepared and built by the getter


# ---------------------------------------------------------------------- 3. first linearize (VC13)
@gpu
@pytest.mark.parametrize("tag", [s[0] for s in K.FIRST_LINEARIZE_SEARCHES])
def test_first_linearize_bit_for_bit(vc, reg, pair, guesses, tag):
    _, search, radius = next(s for s in K.FIRST_LINEARIZE_SEARCHES if s[0] == tag)
    tgt, srcs = K.batch_clouds(pair)
    use = [k for k, n in enumerate(K.SOURCE_SIZES) if tag != "r4.0" or n in K.R4_SIZES]
    b = _batch(vc, reg, search, radius, optimizer=1, max_iterations=1)
    b.set_clouds(0, [tgt] + [srcs[k] for k in use])
    recs = b.align(_pairs(len(use)), [guesses[k] for k in use])     # grid x is sized by the largest kept source
    g = _single(vc, reg, None, tgt, search, radius)
    pt = {"points": g.getPoints(1)[g.kept(1), :3], "covs": g.covariances(1)[1]}
    for i, k in enumerate(use):
        n = K.SOURCE_SIZES[k]
        g.setInputSource(srcs[k])
        cost, _, _ = g.linearize(guesses[k].astype(np.float64))
        corr = g.voxel_correspondences()
        matched = int((corr >= 0).sum())
        got = b.voxel_correspondences(i)
        o = K.restatement({"points": g.getPoints(0)[g.kept(0), :3], "covs": g.covariances(0)[1]}, pt, search, radius)
        o.update_correspondences(guesses[k].astype(np.float64))
        print(tag, n, "kept", corr.shape, "matched", matched, "cost", cost, "face margin", o.face_margin)
        assert o.face_margin >= K.FACE_MARGIN
        assert matched > 0 and got.shape == corr.shape and np.array_equal(got, corr) and np.array_equal(corr, o.voxel_corr), n
        assert np.float64(recs[i]["final_cost"]).view(np.uint64) == np.float64(cost).view(np.uint64), (n, recs[i]["final_cost"], cost)
        assert int(recs[i]["n_matched"]) == matched
        assert (int(recs[i]["n_linearize"]), int(recs[i]["n_compute_error"]), int(recs[i]["iterations"])) == (1, 0, 0)


# ---------------------------------------------------------------------- 4. align parity (VC14)
@gpu
@pytest.mark.parametrize("optimizer", (0, 1), ids=("lm", "gn"))
@pytest.mark.parametrize("tag", [s[0] for s in K.SEARCHES])
def test_align_parity(vc, reg, scene, pair, guesses, tag, optimizer):
    _, search, radius = next(s for s in K.SEARCHES if s[0] == tag)
    tgt, srcs = K.batch_clouds(pair)
    b = _batch(vc, reg, search, radius, optimizer=optimizer)
    b.set_clouds(0, [tgt] + srcs)
    recs = b.align(_pairs(7), guesses)
    ticks = b.debug_counts()[2]
    g = _single(vc, reg, None, tgt, search, radius, optimizer=optimizer)
    pt = {"points": g.getPoints(1)[g.kept(1), :3], "covs": g.covariances(1)[1]}
    seen, converged = set(), []
    for k, n in enumerate(K.SOURCE_SIZES):
        g.setInputSource(srcs[k])
        T = g.align(guesses[k])
        r, w = recs[k], g.result
        got = _ints(r)
        want = (int(w.converged), w.iterations, w.n_linearize, w.n_compute_error, w.lm_failed, w.n_matched)
        # the restatement over the device's own kept points and covariances: the margin of this very run, and the pose
        o = K.restatement({"points": g.getPoints(0)[g.kept(0), :3], "covs": g.covariances(0)[1]}, pt, search, radius, optimizer=optimizer)
        To = o.align(guesses[k])
        rel = abs(float(r["final_cost"]) - w.final_cost) / w.final_cost
        ulps = np.abs(_T(r).astype(np.float64) - T.astype(np.float64)) / np.spacing(np.maximum(np.abs(_T(r)), np.abs(T.astype(np.float32))))
        te, re_ = scene.pose_error(To, _T(r))
        print(tag, "lm" if optimizer == 0 else "gn", n, "record", got, "cost rel", rel, "T ulps", ulps.max(), "pose", te, re_, "face margin", o.face_margin_min)
        assert o.face_margin_min >= K.FACE_MARGIN
        assert got == want, (n, got, want)
        assert got == (int(o.converged), o.nr_iterations, o.trace.n_linearize, o.trace.n_compute_error, 0, o.n_matched), n
        if got[0]:
            converged.append(n)
            assert rel <= TRACE_TOL, (n, rel)
            assert ulps.max() <= 1.0, (n, ulps.max())
            assert te <= 1e-3 and re_ <= 1e-4, (n, te, re_)
        seen.add((got[2], got[3]))
    assert tuple(converged) == K.CONVERGING[tag]
    assert len(seen) >= 2                      # pairs finished in different ticks
    assert ticks >= max(a + c for a, c in seen)


# ---------------------------------------------------------------------- 5. composition independence (VC15)
@gpu
def test_a_record_is_a_pure_function_of_the_pair(vc, reg, pair, guesses, d1_whole):
    tgt, srcs = K.batch_clouds(pair)
    whole = d1_whole
    assert [int(r["converged"]) for r in whole] == [1 if n in K.CONVERGING["d1"] else 0 for n in K.SOURCE_SIZES]
    b = _batch(vc, reg)
    b.set_clouds(0, [tgt] + srcs)
    pairs = _pairs(7)
    alone = [b.align([pairs[i]], [guesses[i]])[0] for i in range(7)]      # a first align of this handle, then six on a reused one
    rev = b.align(pairs[::-1], guesses[::-1])[::-1]
    again = b.align(pairs, guesses)
    for i in range(7):
        assert whole[i].tobytes() == alone[i].tobytes() == rev[i].tobytes() == again[i].tobytes(), i
    assert b.build_count() == (8, 1)


# ---------------------------------------------------------------------- 6. degenerate pairs (VC14 / VC9)
@gpu
@pytest.mark.parametrize("optimizer", (0, 1), ids=("lm", "gn"))
def test_degenerate_pairs_end_alone(vc, reg, pair, guesses, d1_whole, optimizer):
    tgt, srcs = K.batch_clouds(pair)
    line = pair["line"]
    b = _batch(vc, reg, optimizer=optimizer)
    b.set_clouds(0, [tgt, srcs[0], srcs[3], line])
    g_line = np.eye(4, dtype=np.float32)
    g_line[:3, 3] = (0.5, 0.25, -0.125)
    # a running pair, a pair whose TARGET keeps no point, a pair whose SOURCE keeps none, another running pair
    with_line = b.align([(1, 0), (2, 3), (3, 0), (2, 0)], [guesses[0], g_line, g_line, guesses[3]])
    assert len(b.kept(3)) == 0 and b.voxel_count(3) == 0 and len(b.voxels(3)["counts"]) == 0
    for r in (with_line[1], with_line[2]):
        assert _ints(r) == (0, 0, 1, 0, 0, 0)
        assert np.array_equal(_T(r), g_line) and float(r["final_cost"]) == 0.0
    assert b.voxel_correspondences(2).shape == (0, 1) and (b.voxel_correspondences(1) == -1).all()
    without = b.align([(1, 0), (2, 0)], [guesses[0], guesses[3]])
    assert with_line[0].tobytes() == without[0].tobytes() and with_line[3].tobytes() == without[1].tobytes()
    if optimizer == 0:
        assert without[0].tobytes() == d1_whole[0].tobytes() and without[1].tobytes() == d1_whole[3].tobytes()
    assert int(without[0]["converged"]) == 1 and int(without[0]["n_matched"]) > 500


# ---------------------------------------------------------------------- 7. refusals
@gpu
def test_too_few_points_and_a_refused_target(vc, reg, pair, guesses, d1_whole):
    tgt, srcs = K.batch_clouds(pair)
    b = _batch(vc, reg)
    b.set_clouds(0, [tgt] + srcs + [pair["source"][:19]])
    with pytest.raises(reg.ApdgicpError) as ei:
        b.align(_pairs(7) + [(8, 0)], guesses + [guesses[0]])
    assert ei.value.code == -4 and "slot 8" in str(ei.value), str(ei.value)
    assert b.build_count() == (0, 0)                          # no pair has run, nothing was launched
    assert b.align(_pairs(7), guesses).tobytes() == d1_whole.tobytes()      # the handle stays usable: the usual bytes
    # a source of 20 .. k_correspondences - 1 points aligns: the APD covariances are not asked for (sources 6: 20 points, k = 20 default)
    small = _batch(vc, reg, k_correspondences=30)
    small.set_clouds(0, [tgt, srcs[6]])
    assert small.align([(1, 0)], [guesses[6]])[0].tobytes() == d1_whole[6].tobytes()
    # a kept target point beyond 2^20 voxels
    bad = K.refused_target(pair)
    b.set_cloud(8, bad)
    kept = b.kept(8)
    assert 2048 in kept and int(np.nonzero(kept == 2048)[0][0]) < 2048
    for call in (lambda: b.align([(1, 0), (1, 8)], guesses[:2]), lambda: b.voxels(8), lambda: b.voxel_count(8)):
        with pytest.raises(reg.ApdgicpError) as ei:
            call()
        assert ei.value.code == -1 and "point 2048 " in str(ei.value) and "slot 8" in str(ei.value), str(ei.value)
    assert b.align(_pairs(7), guesses).tobytes() == d1_whole.tobytes()


# ---------------------------------------------------------------------- 8. cache rules and mode rules (VC11 / VC12 / VC16)
@gpu
def test_cache_rules(vc, reg, pair, guesses, d1_whole):
    tgt, srcs = K.batch_clouds(pair)
    b = _batch(vc, reg)
    b.set_clouds(0, [tgt, pair["target"][:1024]] + srcs)
    pairs, gs = [(2, 0), (3, 1), (4, 1)], [guesses[0], guesses[1], guesses[2]]      # three pairs, two distinct targets
    first = b.align(pairs, gs)
    assert first[0].tobytes() == d1_whole[0].tobytes()
    assert b.build_count() == (5, 2) and b.debug_counts()[:2] == (1, 1)
    assert b.align(pairs, gs).tobytes() == first.tobytes()
    assert b.build_count() == (5, 2) and b.debug_counts()[:2] == (1, 1)             # unchanged slots: nothing rebuilt, no wait
    b.set_cloud(1, pair["target"][:1023])                                           # a target: its preparation and its map
    b.align(pairs, gs)
    assert b.build_count() == (6, 3) and b.debug_counts()[:2] == (2, 2)
    b.set_cloud(3, srcs[1][:1000])                                                  # a source: its preparation only
    b.align(pairs, gs)
    assert b.build_count() == (7, 3) and b.debug_counts()[:2] == (3, 2)
    b.setNeighborSearchMethod(vc.DIRECT_RADIUS, 1.5)                                # the search is no property of either
    b.align(pairs, gs)
    assert b.build_count() == (7, 3)
    b.setResolution(0.5)                                                            # the maps of the targets USED, no preparation
    b.align(pairs[:1], gs[:1])
    assert b.build_count() == (7, 4)
    b.align(pairs, gs)
    assert b.build_count() == (7, 5) and b.debug_counts()[0] == 3
    b.disable()
    b.enable()
    b.align(pairs, gs)
    assert b.build_count() == (7, 5)                                                # off and on, nothing else changed
    b.setRegularizationMethod(vc.MIN_EIG)                                           # both, of the slots used
    b.align(pairs, gs)
    assert b.build_count() == (12, 7)
    b.setRegularizationMethod(vc.PLANE)
    b.setResolution(1.0)
    b.setNeighborSearchMethod(vc.DIRECT1)
    b.clear()                                                                       # apdgicp_batch_clear drops everything
    b.set_clouds(0, [tgt, pair["target"][:1024]] + srcs)
    assert b.align(pairs, gs).tobytes() == first.tobytes()
    assert b.build_count() == (17, 9)


@gpu
def test_mode_rules(vc, reg, scene, pair, guesses):
    import ctypes as C
    vg = importlib.import_module("riv-slam_amd.vgicp")
    ndt = importlib.import_module("riv-slam_amd.ndt")
    icp = importlib.import_module("riv-slam_amd.icp")
    tgt, srcs = K.batch_clouds(pair)
    b = _batch(vc, reg)
    L = b.L

    def on(getter):
        e = C.c_int()
        assert getter(b.b, None, C.byref(e)) == 0
        return bool(e.value)

    def state():
        return (on(L.apdgicp_batch_get_vgicp_cuda), on(L.apdgicp_batch_get_vgicp), on(L.apdgicp_batch_get_ndt), on(L.apdgicp_batch_get_icp))

    assert state() == (True, False, False, False) and b.enabled()
    p, enabled = b.get_mode()
    assert enabled and (p.resolution, p.neighbor_search, p.regularization) == (1.0, vc.DIRECT1, vc.PLANE)
    with pytest.raises(reg.ApdgicpError) as ei:
        b.setRegularizationMethod(vc.NONE)
    assert ei.value.code == -5 and b.vparams.regularization == vc.PLANE and b.get_mode()[0].regularization == vc.PLANE
    vp = vg.default_vgicp_params()
    assert L.apdgicp_batch_set_vgicp(b.b, C.byref(vp)) == 0 and state() == (False, True, False, False)
    b.enable()
    assert state() == (True, False, False, False)
    np_ = ndt.default_ndt_params()
    assert L.apdgicp_batch_set_ndt(b.b, C.byref(np_)) == 0 and state() == (False, False, True, False)
    b.enable()
    assert state() == (True, False, False, False)
    ip = icp.default_icp_params()
    ip.enable = 1
    assert L.apdgicp_batch_set_icp(b.b, C.byref(ip)) == 0 and state() == (False, False, False, True)
    b.enable()
    assert state() == (True, False, False, False)
    assert L.apdgicp_batch_is_pooled(b.b) == 0
    b.set_pair_groups(2)   # accepted, no effect
    # one batch at a time
    b.set_clouds(0, [tgt, srcs[3], srcs[4]])
    with pytest.raises(reg.ApdgicpError) as ei:
        b.align_enqueue([(1, 0)], [guesses[3]])
    assert ei.value.code == -5 and "apdgicp_batch_set_vgicp_cuda" in str(ei.value)
    assert L.apdgicp_batch_pump(b.b) == -5
    assert L.apdgicp_batch_align_collect(b.b, 1, None, None) == -5
    ptr, nbytes = b.align_async([(1, 0)], [guesses[3]])            # complete on return
    assert ptr and nbytes == 96
    out = np.zeros(1, dtype=reg.RESULT_DTYPE)
    b.copy_results_to(out, 1)
    b.synchronize()
    assert out.tobytes() == b.align([(1, 0)], [guesses[3]]).tobytes()
    # the getters need the mode on
    b.disable()
    assert state() == (False, False, False, False)
    for call in (lambda: b.kept(0), lambda: b.voxel_count(0), lambda: b.voxel_correspondences(0)):
        with pytest.raises(reg.ApdgicpError) as ei:
            call()
        assert ei.value.code == -3
    # mode off: an APD batch as on a handle that never had the mode on
    pairs, gs = [(1, 0), (2, 0)], [guesses[3], guesses[4]]
    apd = b.align(pairs, gs)
    ref = reg.BatchAPDGICP(reg.default_params())
    ref.set_clouds(0, [tgt, srcs[3], srcs[4]])
    assert ref.align(pairs, gs).tobytes() == apd.tobytes()
    t = b.align_enqueue(pairs, gs)                                 # the APD path offers it again
    assert len(b.align_collect(t)) == 2


# ---------------------------------------------------------------------- 9. consumers
@gpu
def test_verify_candidates_picks_what_a_loop_of_one_handle_picks(vc, reg, scene, pair, guesses):
    lv = importlib.import_module("riv-slam_amd.loop_verifier")
    tgt, srcs = K.batch_clouds(pair)
    cands, gs = srcs[:6], guesses[:6]
    b = _batch(vc, reg, vc.DIRECT_RADIUS, 1.5)                     # every pair of this search converges
    thresh = 5.0
    loop, scores, results = lv.verify_candidates(b, tgt, cands, gs, fitness_score_thresh=thresh)
    g = _single(vc, reg, None, tgt, vc.DIRECT_RADIUS, 1.5)
    best_score, best, best_T = np.finfo(np.float64).max, -1, None
    for i, (c, guess) in enumerate(zip(cands, gs)):
        g.setInputSource(c)
        T = g.align(guess)
        score = g.getFitnessScore()
        ulps = np.abs(_T(results[i]).astype(np.float64) - T.astype(np.float64)) / np.spacing(np.maximum(np.abs(_T(results[i])), np.abs(T.astype(np.float32))))
        print(i, len(c), "score", scores[i], score, "T ulps", ulps.max())
        assert ulps.max() <= 1.0 and bool(results[i]["converged"]) == g.hasConverged()
        assert abs(scores[i] - score) <= 1e-3 * score
        if not g.hasConverged() or score > best_score:
            continue
        best_score, best, best_T = score, i, T
    print("scores", scores, "best", best)
    assert best >= 0 and best_score <= thresh and len(set(np.round(scores, 6))) == 6
    assert loop is not None and loop.candidate == best
    assert abs(loop.fitness_score - best_score) <= 1e-3 * best_score
    lT = np.asarray(loop.relative_pose, dtype=np.float32)
    assert (np.abs(lT.astype(np.float64) - best_T.astype(np.float64)) <= np.spacing(np.maximum(np.abs(lT), np.abs(best_T.astype(np.float32))))).all()
    assert b.build_count() == (7, 1)
