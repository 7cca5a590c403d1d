"""NDT (P2D / D2D) as a mode of the BATCH handle: include/apdgicp_hip.h N10 .. N15, riv-slam_amd/csrc/apd_ndt_batch.hpp,
riv-slam_amd/ndt.py (BatchNDT), against the single handle (tests/test_ndt.py checks that one against the restatement) and the
restatement tests/ndt_np.py itself.

CPU part: exports, the Python class, the argument checks that need no handle, and the conditions of every align fixture used below.
GPU part (-m gpu): parameters and exclusivity, maps bit for bit, the first linearize bit for bit, align parity, purity (N14), N8 inside
a batch, clouds smaller than k_correspondences (N11), refusals, the cache rules, the calls the mode does not offer, and loop
verification through loop_verifier.verify_candidates.

Bars.  Maps, the first linearize and everything compared batch against batch: bytes.  Align against the single handle: the integer
fields equal, final_cost 1e-11 relative (the project's TRACE_TOL), every element of T within one float ulp; against the restatement
(handed the device's maps) 1e-3 m / 1e-4 rad.  The integer fields can be exact because sin / cos of the step (device library here, the
host's there) move an iterate in its last bits only and every align fixture keeps its transformed rows >= 1e-9 voxel edges from a
voxel face over the whole run -- asserted on the CPU for each fixture and again for the run the GPU test makes.

How the ALIGN_CASES become batches: a batch handle has ONE set of parameters, so each tuple (x its optimisers) is one batch of six
pairs against the tuple's target: the first n, n/2, n/4+1, n/8+1, n/16+1, n/32+1 points of the tuple's source, each from its own
perturbed guess, so that pairs of different sizes finish after different numbers of iterations and idle beside running ones.
"""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest

import apdgicp_np as anp
import ndt_np as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACE_TOL = 1e-11
FACE_MARGIN = 1e-9
NEW_SYMBOLS = ("apdgicp_batch_set_ndt", "apdgicp_batch_get_ndt", "apdgicp_batch_ndt_voxel_count", "apdgicp_batch_ndt_get_voxels",
               "apdgicp_batch_ndt_build_count")
LM, GN = 0, 1
# (name, pair size, resolution, distance mode, search, optimisers): sources scene.make_pair(n, n, pair_seed(9, 0), "odometry")
ALIGN_CASES = (
    ("d2d_d7_res2", 4099, 2.0, N.D2D, N.DIRECT7, (LM, GN)),
    ("p2d_d1_res2", 4099, 2.0, N.P2D, N.DIRECT1, (LM, GN)),
    ("p2d_d7_res2", 4099, 2.0, N.P2D, N.DIRECT7, (LM, GN)),
    ("d2d_d27_res2", 4099, 2.0, N.D2D, N.DIRECT27, (LM,)),
    ("d2d_d1", 8192, 1.0, N.D2D, N.DIRECT1, (LM, GN)),
    ("d2d_d7", 8192, 1.0, N.D2D, N.DIRECT7, (LM, GN)),
)
CASE_OPT = [(c[0], o) for c in ALIGN_CASES for o in c[5]]
CASE_OPT_IDS = [f"{n}-{'lm' if o == LM else 'gn'}" for n, o in CASE_OPT]
INT_FIELDS = ("converged", "iterations", "n_linearize", "n_compute_error", "lm_failed", "n_matched")
_CPU_RUNS = {}


@pytest.fixture(scope="module")
def reg():
    import __graft_entry__ as g
    g.build()
    return importlib.import_module("riv-slam_amd.registration")


@pytest.fixture(scope="module")
def nd(reg):
    return importlib.import_module("riv-slam_amd.ndt")


def _variant_sizes(n):
    return (n, n // 2, n // 4 + 1, n // 8 + 1, n // 16 + 1, n // 32 + 1)


def _case_pairs(scene, name):
    """The six pairs of one tuple's batch: (resolution, mode, search, target, [(source, guess)])."""
    tag, n, res, mode, search, _ = next(c for c in ALIGN_CASES if c[0] == name)
    src, tgt, _, guess = scene.make_pair(n, n, scene.pair_seed(9, 0), "odometry")
    pairs = []
    for k, m in enumerate(_variant_sizes(n)):
        P = scene.make_transform(np.array([0.04 * k, -0.03 * k, 0.01 * k]), 0.003 * k, 0.0, 0.0)
        pairs.append((src[:m], (P @ guess.astype(np.float64)).astype(np.float32)))
    return res, mode, search, tgt, pairs


# ====================================================================== CPU
def test_new_symbols_are_exported_and_the_class_imports(reg, nd):
    L = reg.load_library()
    header = open(os.path.join(ROOT, "include", "apdgicp_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), f"{name} is not exported"
        assert name in reg.SYMBOLS
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared"
    assert "Batch handles have no NDT mode" not in header
    for v in ("N10.", "N11.", "N12.", "N13.", "N14.", "N15."):
        assert v in header
    assert L.apdgicp_abi_version() == 6


def test_batch_ndt_class(reg, nd):
    assert issubclass(nd.BatchNDT, reg.BatchAPDGICP)
    for m in ("setDistanceMode", "setResolution", "setNeighborSearchMethod", "get_ndt", "enable", "disable", "enabled", "voxel_count", "voxels", "build_count",
              "align", "align_async", "synchronize", "fitness", "set_clouds"):
        assert callable(getattr(nd.BatchNDT, m))


def test_set_ndt_checks_its_parameters_before_anything_else(reg, nd):
    """The parameter checks need no handle: DIRECT_RADIUS is refused as UNSUPPORTED, a resolution that is not positive, an unknown search
    method and an unknown distance mode as INVALID_ARG; valid parameters reach the handle check (INVALID_ARG: the handle is null)."""
    L = reg.load_library()
    p = nd.default_ndt_params()
    assert L.apdgicp_batch_set_ndt(None, ctypes.byref(p)) == -1
    p.neighbor_search = nd.DIRECT_RADIUS
    assert L.apdgicp_batch_set_ndt(None, ctypes.byref(p)) == -5
    p = nd.default_ndt_params()
    p.resolution = 0.0
    assert L.apdgicp_batch_set_ndt(None, ctypes.byref(p)) == -1
    p = nd.default_ndt_params()
    p.neighbor_search = 4
    assert L.apdgicp_batch_set_ndt(None, ctypes.byref(p)) == -1
    p = nd.default_ndt_params()
    p.distance_mode = 2
    assert L.apdgicp_batch_set_ndt(None, ctypes.byref(p)) == -1
    n = ctypes.c_int64()
    assert L.apdgicp_batch_ndt_build_count(None, ctypes.byref(n)) == -1
    assert L.apdgicp_batch_ndt_voxel_count(None, 0, ctypes.byref(n)) == -1
    assert L.apdgicp_batch_ndt_get_voxels(None, 0, 0, None, None, None, None, None) == -1
    assert L.apdgicp_batch_get_ndt(None, None, None) == -1


@pytest.mark.parametrize("name", [c[0] for c in ALIGN_CASES])
def test_align_fixtures_meet_the_conditions_of_exact_comparison(scene, name):
    """The conditions under which integer fields can be compared exactly, with the restatement alone (its own maps), for every pair and
    optimiser of every batch of test_align_parity -- the smaller variants included."""
    res, mode, search, tgt, pairs = _case_pairs(scene, name)
    tmap = N.build_map(tgt, res)
    for optimizer in next(c[5] for c in ALIGN_CASES if c[0] == name):
        iterations = []
        for src, guess in pairs:
            o = N.NDT(anp.Params(optimizer=optimizer), resolution=res, distance_mode=mode, search=search)
            o.setInputSource(src)
            o.setInputTarget(tgt)
            o.set_maps(tmap, N.build_map(src, res, "source") if mode == N.D2D else None)
            o.align(guess)
            print(name, optimizer, len(src), "iterations", o.nr_iterations, "n_matched", o.n_matched, "face margin", o.face_margin_min)
            assert o.face_margin_min >= FACE_MARGIN, (len(src), optimizer, o.face_margin_min)
            assert o.converged and o.n_matched >= 80 and o.nr_iterations <= 30, (len(src), optimizer, o.converged, o.n_matched, o.nr_iterations)
            iterations.append(o.nr_iterations)
        assert len(set(iterations)) >= 2, iterations   # the pairs of a batch do not all stop at the same iteration


# ====================================================================== GPU
gpu = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _assert_map_equal(got, want):
    assert np.array_equal(got["coords"], want["coords"])
    assert np.array_equal(got["counts"], want["counts"])
    for k in ("means", "raw", "covs"):
        assert np.array_equal(_bits(got[k]), _bits(want[k])), k


def _scene_cloud(n, seed=21):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(n, 3)) * [7, 7, 1.5]).astype(np.float32)


def _lattice_source(tgt, res, nv, seed=17):
    """A source with exactly nv voxels: one to three points well inside each of nv cells of the target's map, the fullest cells first"""
    rng = np.random.default_rng(seed)
    m = N.build_map(tgt, res)
    cells = m["coords"][np.argsort(-m["counts"], kind="stable")[:nv]].astype(np.float64)
    assert len(cells) == nv
    pts = []
    for c in cells:
        for _ in range(int(rng.integers(1, 4))):
            pts.append((c + 1.0 + rng.uniform(-0.3, 0.3, size=3)) * res)
    pts = np.array(pts, dtype=np.float32)
    return pts[rng.permutation(len(pts))]


def _one_point_per_voxel(res, half=6):
    """A target whose every voxel holds one point (the centre of its cell): no voxel passes the gate at six points"""
    c = np.arange(-half, half, dtype=np.float64)
    g = np.stack(np.meshgrid(c, c, c[half - 2:half + 2], indexing="ij"), axis=-1).reshape(-1, 3)
    return ((g + 1.0) * res).astype(np.float32)


def _T(rec):
    return np.asarray(rec["T"], dtype=np.float32).reshape(4, 4).T


def _ints(rec):
    return tuple(int(rec[k]) for k in INT_FIELDS)


def _batch(reg, nd, mode=N.D2D, search=N.DIRECT7, res=1.0, **kw):
    b = nd.BatchNDT(reg.default_params(**kw))
    b.setResolution(res)
    b.setDistanceMode(mode)
    b.setNeighborSearchMethod(search)
    return b


def _single(reg, nd, src, tgt, mode=N.D2D, search=N.DIRECT7, res=1.0, **kw):
    g = nd.NDT(reg.default_params(**kw))
    g.setResolution(res)
    g.setDistanceMode(mode)
    g.setNeighborSearchMethod(search)
    g.setInputSource(src)
    g.setInputTarget(tgt)
    return g


def _assert_record_close(r, g, T):
    """The bars of the align parity test, batch record r against the single handle g after its align returned T."""
    w = g.result
    want = (int(w.converged), w.iterations, w.n_linearize, w.n_compute_error, w.lm_failed, w.n_matched)
    rel = abs(float(r["final_cost"]) - w.final_cost) / w.final_cost if w.final_cost != 0.0 else abs(float(r["final_cost"]))
    ulps = np.abs(_T(r).astype(np.float64) - T.astype(np.float64)) / np.spacing(np.maximum(np.abs(_T(r)), np.abs(T.astype(np.float32))))
    print("record", _ints(r), "single", want, "cost rel", rel, "T ulps", ulps.max())
    assert _ints(r) == want, (_ints(r), want)
    assert rel <= TRACE_TOL
    assert ulps.max() <= 1.0
    return rel, ulps.max()


# ---------------------------------------------------------------------- 1. parameters
@gpu
def test_params_round_trip_and_exclusivity(reg, nd):
    vg = importlib.import_module("riv-slam_amd.vgicp")
    b = nd.BatchNDT()
    p, on = b.get_ndt()
    assert on and b.enabled() and (p.resolution, p.distance_mode, p.neighbor_search) == (1.0, nd.D2D, nd.DIRECT7)
    b.setResolution(0.75)
    b.setDistanceMode(nd.P2D)
    b.setNeighborSearchMethod(nd.DIRECT27)
    p, on = b.get_ndt()
    assert on and (p.resolution, p.distance_mode, p.neighbor_search) == (0.75, nd.P2D, nd.DIRECT27)
    with pytest.raises(reg.ApdgicpError) as ei:
        b.setNeighborSearchMethod(nd.DIRECT_RADIUS)
    assert ei.value.code == -5
    p, on = b.get_ndt()
    assert on and p.neighbor_search == nd.DIRECT27 and b.nparams.neighbor_search == nd.DIRECT27
    # exclusive with the voxelized GICP mode, in both directions
    vp, von = vg.VgicpParams(), ctypes.c_int()
    assert b.L.apdgicp_batch_get_vgicp(b.b, ctypes.byref(vp), ctypes.byref(von)) == 0 and von.value == 0
    vp = vg.default_vgicp_params()
    assert b.L.apdgicp_batch_set_vgicp(b.b, ctypes.byref(vp)) == 0
    assert not b.enabled() and b.get_ndt()[0].resolution == 0.75
    assert b.L.apdgicp_batch_get_vgicp(b.b, ctypes.byref(vp), ctypes.byref(von)) == 0 and von.value == 1
    b.enable()
    assert b.enabled()
    assert b.L.apdgicp_batch_get_vgicp(b.b, ctypes.byref(vp), ctypes.byref(von)) == 0 and von.value == 0
    b.disable()
    assert not b.enabled() and b.get_ndt()[0].resolution == 0.75
    with pytest.raises(reg.ApdgicpError) as ei:
        b.voxel_count(0)
    assert ei.value.code == -3
    b.enable()
    assert b.enabled()


# ---------------------------------------------------------------------- 2. maps (N10)
@gpu
def test_maps_bit_for_bit_and_one_build_per_distinct_slot(reg, nd):
    sizes = (7, 64, 65, 257, 4099)
    clouds = [_scene_cloud(n) for n in sizes]
    b = _batch(reg, nd)
    b.set_clouds(0, clouds)
    assert b.build_count() == 0
    for t, cloud in enumerate(clouds):
        g = nd.NDT()
        g.setInputTarget(cloud)
        _assert_map_equal(b.voxels(t), g.voxels(reg.TARGET))
        assert b.voxel_count(t) == g.voxel_count(reg.TARGET)
    assert b.build_count() == 5                      # one per slot asked for, the second getter found each there
    pairs = [(0, 4), (1, 4), (4, 0)]
    d = _batch(reg, nd, N.D2D)
    d.set_clouds(0, clouds)
    d.align(pairs)
    assert d.build_count() == 3                      # D2D: every distinct slot used, as a source or as a target (0, 1, 4)
    p = _batch(reg, nd, N.P2D)
    p.set_clouds(0, clouds)
    p.align(pairs)
    assert p.build_count() == 2                      # P2D: the distinct targets (4, 0)
    _assert_map_equal(p.voxels(4), b.voxels(4))
    assert p.build_count() == 2 and p.voxel_count(1) > 0 and p.build_count() == 3   # a source-only slot had none until it was asked for


# ---------------------------------------------------------------------- 3. first linearize (N12)
@pytest.fixture(scope="module")
def lin_pair(scene):
    src, tgt, _, guess = scene.make_pair(2048, 4099, scene.pair_seed(0, 0), "odometry")
    return src, tgt, guess


@gpu
@pytest.mark.parametrize("mode", (N.P2D, N.D2D), ids=("p2d", "d2d"))
@pytest.mark.parametrize("search", (0, 1, 2))
def test_first_linearize_bit_for_bit(reg, nd, lin_pair, search, mode):
    """One batch whose row counts straddle the block edges (D2D: sources of exactly 1, 64, 65, 256 and 257 voxels; P2D: 20, 64, 65, 256
    and 257 points) beside a 2048-point pair that sizes the grid; Gauss-Newton, one iteration: the record's cost is the first linearize's."""
    src, tgt, guess = lin_pair
    rows = (1, 64, 65, 256, 257) if mode == N.D2D else (20, 64, 65, 256, 257)
    sources = [_lattice_source(tgt, 1.0, nv) if mode == N.D2D else src[:nv] for nv in rows] + [src]
    b = _batch(reg, nd, mode, search, optimizer=GN, max_iterations=1)
    b.set_clouds(0, [tgt] + sources)
    recs = b.align([(1 + i, 0) for i in range(len(sources))], [guess] * len(sources))
    for i, s in enumerate(sources):
        g = _single(reg, nd, s, tgt, mode, search)
        cost, _, _ = g.linearize(guess.astype(np.float64))
        corr = g.voxel_correspondences()
        counts = g.voxels(reg.TARGET)["counts"]
        matched = int(((corr >= 0) & (counts[np.maximum(corr, 0)] > 6)).sum())
        if i < len(rows):
            assert len(corr) == rows[i] and (mode == N.P2D or b.voxel_count(1 + i) == rows[i])
        assert matched > 0
        assert np.float64(recs[i]["final_cost"]).view(np.uint64) == np.float64(cost).view(np.uint64), (i, recs[i]["final_cost"], cost)
        assert int(recs[i]["n_matched"]) == matched
        assert (int(recs[i]["n_linearize"]), int(recs[i]["n_compute_error"])) == (1, 0)


# ---------------------------------------------------------------------- 4. align parity (N13)
@gpu
@pytest.mark.parametrize("name,optimizer", CASE_OPT, ids=CASE_OPT_IDS)
def test_align_parity(reg, nd, scene, name, optimizer):
    res, mode, search, tgt, pairs = _case_pairs(scene, name)
    b = _batch(reg, nd, mode, search, res, optimizer=optimizer)
    b.set_clouds(0, [tgt] + [s for s, _ in pairs])
    recs = b.align([(1 + i, 0) for i in range(len(pairs))], [g for _, g in pairs])
    ticks = b.last_ticks()[0]
    tmap = N.map_from_device(b.voxels(0))
    seen = set()
    g = nd.NDT(reg.default_params(optimizer=optimizer))     # ONE single handle, looped over the pairs
    g.setResolution(res)
    g.setDistanceMode(mode)
    g.setNeighborSearchMethod(search)
    g.setInputTarget(tgt)
    for i, (src, guess) in enumerate(pairs):
        g.setInputSource(src)
        T = g.align(guess)
        r = recs[i]
        # the restatement with the device's maps: the margin of this very run, and the pose
        o = N.NDT(anp.Params(optimizer=optimizer), resolution=res, distance_mode=mode, search=search)
        o.setInputSource(src)
        o.setInputTarget(tgt)
        o.set_maps(tmap, N.map_from_device(b.voxels(1 + i)) if mode == N.D2D else None)
        To = o.align(guess)
        te, re_ = scene.pose_error(To, _T(r))
        print(name, "lm" if optimizer == LM else "gn", len(src), "pose", te, re_, "face margin", o.face_margin_min)
        assert o.face_margin_min >= FACE_MARGIN
        _assert_record_close(r, g, T)
        assert _ints(r) == (int(o.converged), o.nr_iterations, o.trace.n_linearize, o.trace.n_compute_error, 0, o.n_matched)
        assert te <= 1e-3 and re_ <= 1e-4
        seen.add((int(r["n_linearize"]), int(r["n_compute_error"])))
    assert len(seen) >= 2                      # pairs finished in different ticks
    assert ticks >= max(a + c for a, c in seen)


# ---------------------------------------------------------------------- 5. purity (N14)
@gpu
@pytest.mark.parametrize("mode", (N.P2D, N.D2D), ids=("p2d", "d2d"))
def test_a_record_is_a_pure_function_of_the_pair(reg, nd, scene, mode):
    name = "d2d_d7_res2" if mode == N.D2D else "p2d_d7_res2"
    res, _, search, tgt, pairs = _case_pairs(scene, name)
    b = _batch(reg, nd, mode, search, res)
    b.set_clouds(0, [tgt] + [s for s, _ in pairs])
    ids = [(1 + i, 0) for i in range(6)]
    guesses = [g for _, g in pairs]
    whole = b.align(ids, guesses)
    assert sum(int(r["converged"]) for r in whole) == 6 and len({int(r["n_linearize"]) for r in whole}) >= 2
    rev = b.align(ids[::-1], guesses[::-1])[::-1]
    again = b.align(ids, guesses)
    for i in range(6):
        alone = b.align([ids[i]], [guesses[i]])[0]
        assert whole[i].tobytes() == rev[i].tobytes() == again[i].tobytes() == alone.tobytes(), i
    # the target also serves as another pair's source: (a -> b) and (b -> a) in one batch
    back = np.linalg.inv(guesses[0].astype(np.float64)).astype(np.float32)
    both = b.align([(1, 0), (0, 1)], [guesses[0], back])
    assert both[0].tobytes() == whole[0].tobytes()
    assert both[1].tobytes() == b.align([(0, 1)], [back])[0].tobytes() and int(both[1]["n_linearize"]) >= 1
    # a first align on another handle, and the same handle after an align of larger clouds in the same slots (stale indices, rows, counts)
    fresh = _batch(reg, nd, mode, search, res)
    fresh.set_clouds(0, [tgt, pairs[2][0]])
    assert fresh.align([(1, 0)], [guesses[2]])[0].tobytes() == whole[2].tobytes()
    big_src, big_tgt, _, big_guess = scene.make_pair(8192, 8192, scene.pair_seed(9, 1), "odometry")
    fresh.set_clouds(0, [big_tgt, big_src])
    assert int(fresh.align([(1, 0), (0, 1)], [big_guess, big_guess])[0]["n_linearize"]) >= 1
    fresh.set_clouds(0, [tgt, pairs[2][0]])
    assert fresh.align([(1, 0)], [guesses[2]])[0].tobytes() == whole[2].tobytes()
    fresh.set_clouds(0, [tgt, pairs[5][0]])
    assert fresh.align([(1, 0)], [guesses[5]])[0].tobytes() == whole[5].tobytes()


# ---------------------------------------------------------------------- 6. N8 inside a batch
@gpu
@pytest.mark.parametrize("mode", (N.P2D, N.D2D), ids=("p2d", "d2d"))
@pytest.mark.parametrize("optimizer", (LM, GN), ids=("lm", "gn"))
def test_pairs_without_a_contributing_term_end_alone(reg, nd, scene, optimizer, mode):
    res, _, search, tgt, pairs = _case_pairs(scene, "d2d_d7_res2")
    (src, guess), (src2, guess2) = pairs[0], pairs[2]
    far = src[:257] + np.float32(500.0)
    g_far = np.eye(4, dtype=np.float32)
    g_far[:3, 3] = (0.5, 0.25, -0.125)
    sparse = _one_point_per_voxel(res)
    b = _batch(reg, nd, mode, search, res, optimizer=optimizer)
    b.set_clouds(0, [tgt, src, far, src2, sparse])
    assert b.voxels(4)["counts"].max() == 1
    mixed = b.align([(1, 0), (2, 0), (3, 0), (3, 4)], [guess, g_far, guess2, guess2])
    for r, g0 in ((mixed[1], g_far), (mixed[3], guess2)):
        assert _ints(r) == (0, 0, 1, 0, 0, 0)
        assert np.array_equal(_T(r), g0) and float(r["final_cost"]) == 0.0
    without = b.align([(1, 0), (3, 0)], [guess, guess2])
    assert mixed[0].tobytes() == without[0].tobytes() and mixed[2].tobytes() == without[1].tobytes()
    assert int(without[0]["converged"]) == 1 and int(without[0]["n_matched"]) >= 80


# ---------------------------------------------------------------------- 7. N11
@gpu
@pytest.mark.parametrize("mode", (N.P2D, N.D2D), ids=("p2d", "d2d"))
def test_clouds_smaller_than_k_correspondences_align(reg, nd, mode):
    """No k-NN covariances: 7 points against 12 and 12 against 7 with k_correspondences = 20, every cloud one voxel."""
    rng = np.random.default_rng(2)
    c12 = rng.uniform(0.6, 1.4, size=(12, 3)).astype(np.float32)
    c7 = (c12[:7] + np.float32(0.05)).astype(np.float32)
    b = _batch(reg, nd, mode, N.DIRECT1)
    assert b.params.k_correspondences == 20
    b.set_clouds(0, [c7, c12])
    recs = b.align([(0, 1), (1, 0)])
    assert b.voxels(0)["counts"].tolist() == [7] and b.voxels(1)["counts"].tolist() == [12]
    for r, (s, t) in zip(recs, ((c7, c12), (c12, c7))):
        g = _single(reg, nd, s, t, mode, N.DIRECT1)
        T = g.align()
        assert np.isfinite(_T(r)).all() and int(r["n_linearize"]) >= 1 and int(r["n_matched"]) == (len(s) if mode == N.P2D else 1)
        if mode == N.P2D:     # (D2D: ONE term, a rank-3 system -- whatever a solver makes of it is not compared, as on the single handle)
            _assert_record_close(r, g, T)


# ---------------------------------------------------------------------- 8. refusals
@gpu
def test_refused_points_fail_the_align_and_the_handle_stays_usable(reg, nd, scene):
    res, _, search, tgt, pairs = _case_pairs(scene, "d2d_d7_res2")
    src, guess = pairs[2]
    bad_t = tgt[:700].copy()
    bad_t[5, 1] = np.nan
    bad_s = src.copy()
    bad_s[9, 2] = np.nan

    def clean(mode):
        f = _batch(reg, nd, mode, search, res)
        f.set_clouds(0, [tgt, tgt[:700], src])
        return f.align([(2, 0), (2, 1)], [guess, guess])

    for mode in (N.D2D, N.P2D):
        want = clean(mode)
        b = _batch(reg, nd, mode, search, res)
        b.set_clouds(0, [tgt, bad_t, src])
        with pytest.raises(reg.ApdgicpError) as ei:
            b.align([(2, 0), (2, 1)], [guess, guess])
        assert ei.value.code == -1 and "slot 1" in str(ei.value) and "point 5" in str(ei.value)
        b.set_cloud(1, tgt[:700])
        assert b.align([(2, 0), (2, 1)], [guess, guess]).tobytes() == want.tobytes()
        b.set_cloud(2, bad_s)
        if mode == N.D2D:
            with pytest.raises(reg.ApdgicpError) as ei:
                b.align([(2, 0), (2, 1)], [guess, guess])
            assert ei.value.code == -1 and "slot 2" in str(ei.value) and "point 9" in str(ei.value)
        else:                 # P2D: the point is a miss
            recs = b.align([(2, 0), (2, 1)], [guess, guess])
            g = _single(reg, nd, bad_s, tgt, mode, search, res)
            T = g.align(guess)
            _assert_record_close(recs[0], g, T)
        b.set_cloud(2, src)
        assert b.align([(2, 0), (2, 1)], [guess, guess]).tobytes() == want.tobytes()


# ---------------------------------------------------------------------- 9. cache rules
@gpu
def test_cache_rules_and_the_apd_path_is_left_alone(reg, nd, scene):
    srcA, tgtA, _, gA = scene.make_pair(2048, 4099, scene.pair_seed(7, 0), "odometry")
    srcB, tgtB, _, gB = scene.make_pair(2048, 4099, scene.pair_seed(7, 1), "odometry")
    b = _batch(reg, nd, N.D2D, N.DIRECT7, 2.0)
    b.set_clouds(0, [tgtA, tgtB, srcA, srcB])
    pairs, guesses = [(2, 0), (3, 1), (2, 1)], [gA, gB, gA]     # three pairs, four distinct slots
    first = b.align(pairs, guesses)
    assert b.build_count() == 4
    assert b.align(pairs, guesses).tobytes() == first.tobytes() and b.build_count() == 4    # unchanged clouds: no build
    b.set_cloud(1, tgtB[:4000])
    b.align(pairs, guesses)
    assert b.build_count() == 5                                  # exactly the slot that was set again
    b.setNeighborSearchMethod(nd.DIRECT1)                        # the search method is no property of a map
    b.align(pairs, guesses)
    assert b.build_count() == 5
    b.setDistanceMode(nd.P2D)                                    # nor is the distance mode: the targets' maps are there
    b.align(pairs, guesses)
    assert b.build_count() == 5
    b.setDistanceMode(nd.D2D)
    b.setResolution(1.0)
    b.align(pairs[:1], guesses[:1])
    assert b.build_count() == 7                                  # another resolution: exactly the slots USED
    b.align(pairs, guesses)
    assert b.build_count() == 9
    b.disable()
    b.enable()
    again = b.align(pairs, guesses)
    assert b.build_count() == 9                                  # off and on, nothing else changed
    # mode off: an APD batch as on a handle that never had the mode on
    b.disable()
    apd = b.align(pairs, guesses)
    ref = reg.BatchAPDGICP(reg.default_params())
    ref.set_clouds(0, [tgtA, tgtB[:4000], srcA, srcB])
    assert ref.align(pairs, guesses).tobytes() == apd.tobytes()
    assert b.build_count() == 9
    b.enable()
    assert b.align(pairs, guesses).tobytes() == again.tobytes() and b.build_count() == 9
    b.clear()                                                    # apdgicp_batch_clear drops every map
    b.set_clouds(0, [tgtA, tgtB[:4000], srcA, srcB])
    assert b.align(pairs, guesses).tobytes() == again.tobytes()
    assert b.build_count() == 13


@gpu
def test_aligns_across_mode_switches_on_one_handle(reg, nd, scene):
    """One handle through voxelized GICP, NDT, a cloud one point past a radix tile (the shared build scratch grows from one block to two
    between the modes), NDT, voxelized GICP and APD-GICP: every record is byte for byte the record of a fresh handle that only ever ran
    that mode on the same pairs (V11 / N14: a record is a pure function of its pair), and a mode switch rebuilds no current map."""
    vg = importlib.import_module("riv-slam_amd.vgicp")
    src, tgt, _, guess = scene.make_pair(4099, 4099, scene.pair_seed(9, 0), "odometry")
    clouds = [src[:517], src[:1031], tgt]
    near = scene.make_transform(np.array([0.04, -0.03, 0.01]), 0.003, 0.0, 0.0).astype(np.float32)   # prefixes of one cloud: truth is identity
    pairs = [(0, 1), (1, 0), (1, 2)]
    guesses = [near, np.linalg.inv(near.astype(np.float64)).astype(np.float32), guess]
    kw = dict(optimizer=LM)

    fresh_vg = vg.BatchVGICP(reg.default_params(**kw))
    fresh_vg.setResolution(2.0)
    fresh_vg.set_clouds(0, clouds)
    want_vg = fresh_vg.align(pairs, guesses)
    fresh_nd = _batch(reg, nd, N.D2D, N.DIRECT7, 2.0, **kw)
    fresh_nd.set_clouds(0, clouds)
    want_nd = fresh_nd.align(pairs, guesses)
    fresh_apd = reg.BatchAPDGICP(reg.default_params(**kw))
    fresh_apd.set_clouds(0, clouds)
    want_apd = fresh_apd.align(pairs, guesses)
    assert int(want_vg[2]["n_linearize"]) >= 2 and int(want_nd[2]["n_linearize"]) >= 2 and int(want_apd[2]["n_linearize"]) >= 2

    b = _batch(reg, nd, N.D2D, N.DIRECT7, 2.0, **kw)
    vp = vg.default_vgicp_params()
    vp.resolution = 2.0

    def vgicp_on():
        assert b.L.apdgicp_batch_set_vgicp(b.b, ctypes.byref(vp)) == 0 and not b.enabled()

    def builds():
        n = ctypes.c_int64()
        assert b.L.apdgicp_batch_vgicp_build_count(b.b, ctypes.byref(n)) == 0
        return n.value, b.build_count()

    def same(got, want):
        assert len(got) == len(want)
        for i in range(len(got)):
            assert got[i].tobytes() == want[i].tobytes(), i

    b.set_clouds(0, clouds[:2])
    vgicp_on()
    same(b.align(pairs[:2], guesses[:2]), want_vg[:2])
    assert builds() == (2, 0)                                    # voxelized GICP maps the targets: slots 1 and 0
    b.enable()
    same(b.align(pairs[:2], guesses[:2]), want_nd[:2])
    assert builds() == (2, 2)                                    # D2D maps sources and targets: slots 0 and 1
    assert b.add_cloud(clouds[2]) == 2
    same(b.align(pairs, guesses), want_nd)
    assert builds() == (2, 3)                                    # only the new slot
    vgicp_on()
    same(b.align(pairs, guesses), want_vg)
    assert builds() == (3, 3)                                    # only the new target; slots 0 and 1 kept their maps through the NDT aligns
    assert b.L.apdgicp_batch_set_vgicp(b.b, None) == 0 and not b.enabled()
    same(b.align(pairs, guesses), want_apd)
    assert builds() == (3, 3)


# ---------------------------------------------------------------------- 10. unsupported calls
@gpu
def test_enqueue_is_unsupported_with_the_mode_on(reg, nd, scene):
    src, tgt, _, guess = scene.make_pair(257, 700, scene.pair_seed(7, 0), "odometry")
    b = _batch(reg, nd, N.D2D, N.DIRECT7, 2.0)
    b.set_clouds(0, [tgt, src])
    with pytest.raises(reg.ApdgicpError) as ei:
        b.align_enqueue([(1, 0)], [guess])
    assert ei.value.code == -5 and "apdgicp_batch_set_ndt" in str(ei.value)
    assert b.L.apdgicp_batch_pump(b.b) == -5
    assert b.L.apdgicp_batch_align_collect(b.b, 1, None, None) == -5
    assert b.L.apdgicp_batch_is_pooled(b.b) == 0
    b.set_pair_groups(2)   # accepted, no effect
    ptr, nbytes = b.align_async([(1, 0)], [guess])            # complete on return
    assert ptr and nbytes == 96
    out = np.zeros(1, dtype=reg.RESULT_DTYPE)
    b.copy_results_to(out, 1)
    b.synchronize()
    assert out.tobytes() == b.align([(1, 0)], [guess]).tobytes()
    b.disable()
    t = b.align_enqueue([(1, 0)], [guess])                    # the APD path offers it again
    assert len(b.align_collect(t)) == 1


# ---------------------------------------------------------------------- 11. consumers
@gpu
def test_verify_candidates_picks_what_a_loop_of_single_handles_picks(reg, nd, scene):
    lv = importlib.import_module("riv-slam_amd.loop_verifier")
    # the new keyframe (the scan) is the TARGET, the six keyframes before it are the candidates (loop_detector.cpp:392-411)
    tgt, cands, _, to_keyframe = scene.make_keyframe_set(4099, 2048, 6, scene.pair_seed(7, 3))
    guesses = [np.linalg.inv(g.astype(np.float64)).astype(np.float32) for g in to_keyframe]
    b = _batch(reg, nd, N.D2D, N.DIRECT7, 2.0)
    thresh = 2.0
    loop, scores, results = lv.verify_candidates(b, tgt, cands, guesses, fitness_score_thresh=thresh)
    best_score, best = np.finfo(np.float64).max, -1
    for i, (c, guess) in enumerate(zip(cands, guesses)):
        g = _single(reg, nd, c, tgt, N.D2D, N.DIRECT7, 2.0)
        T = g.align(guess)
        score = g.getFitnessScore()
        te, re_ = scene.pose_error(T, _T(results[i]))
        print(i, "converged", bool(results[i]["converged"]), g.hasConverged(), "score", scores[i], score, "pose", te, re_)
        assert bool(results[i]["converged"]) == g.hasConverged()
        if not g.hasConverged() or score > best_score:
            continue
        best_score, best = score, i
    print("scores", scores, "best", best)
    assert (loop.candidate if loop is not None else -1) == (best if best_score <= thresh else -1)
    assert b.build_count() == 7                                  # D2D: the target's map once, one per candidate
