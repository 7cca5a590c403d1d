"""FAST_VGICP_CUDA (fast_gicp::FastVGICPCuda) as a mode of the registration handle, on the GPU: include/apdgicp_hip.h VC1 .. VC10,
riv-slam_amd/csrc/apd_vgicp_cuda.hpp, riv-slam_amd/vgicp_cuda.py, against the restatement tests/vgicp_cuda_np.py.  (The part that needs
no GPU: tests/test_vgicp_cuda_cpu.py.)

Bars: kept lists, voxel correspondences and n_matched exact; raw covariances bit for bit (VC2 has a stated order; the neighbour lists
have no ties in the fixture beyond the (distance, index) order both sides use); regularised covariances 1e-10 times max(1, the largest entry) -- the bar of
tests/test_hip_parity.py for the covariances of the APD path in the form it takes where entries exceed 1 (test_cov_any_k_above_64);
PLANE's entries are below 1, where it is 1e-10 absolute; FROBENIUS's reach 3.2e3 in this fixture, where numpy's own two routes to the
same matrix ((C'^-1 / |C'^-1|)^-1 and C' |C'^-1|) differ by 1.3e-10 absolute and the device measured 1.4e-9; the voxel map bit for bit against the FAST_VGICP mode fed the same kept
points and covariances; H, b, cost 1e-10 relative and every lambda, rho, cost and pose of an optimiser trace 1e-11 (tests/test_vgicp.py's
bars).  Clouds: tests/golden/vgicp_cuda_pair.npz and its prefixes, whose conditions tests/test_vgicp_cuda_cpu.py asserts.
"""
import importlib
import os

import numpy as np
import pytest

import apdgicp_np as anp
import vgicp_cuda_np as VC
import vgicp_np as V
from conftest import rel_err
from trace_util import trace_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COV_TOL = 1e-10
HB_TOL = 1e-10
TRACE_TOL = 1e-11
FACE_MARGIN = 1e-9
SIZES = (20, 21, 63, 64, 65, 255, 256, 257, 2048)
SEARCHES = (("d1", 0, 1.5), ("d7", 1, 1.5), ("d27", 2, 1.5), ("r0", 3, 0.0), ("r1.0", 3, 1.0), ("r1.5", 3, 1.5), ("r4.0", 3, 4.0))
SRC, TGT = 0, 1
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
def vg(reg):
    return importlib.import_module("riv-slam_amd.vgicp")


@pytest.fixture(scope="module")
def pair():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "vgicp_cuda_pair.npz")))


@pytest.fixture(scope="module")
def prepared(pair):
    """the restatement's prepared clouds, computed once per (cloud, size, regularisation) and shared"""
    cache = {}

    def get(name, n, method=VC.PLANE):
        key = (name, n, method)
        if key not in cache:
            cache[key] = VC.prepare(pair[name][:n], method)
        return cache[key]
    return get


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _new(vc, reg, search=0, radius=1.5, regularization=VC.PLANE, res=1.0, **kw):
    g = vc.FastVGICPCuda(reg.default_params(**kw))
    g.setRegularizationMethod(regularization)
    g.setNeighborSearchMethod(search, radius)
    g.setResolution(res)
    return g


def _mirror(g, **kw):
    """The restatement over the device's OWN kept points and covariances (they are compared on their own): what is compared through it is
    everything behind them -- map, offsets, lookup, cost, loop."""
    p = g.vparams
    o = VC.FastVGICPCuda(anp.Params(**kw), p.resolution, p.neighbor_search, p.search_radius, p.regularization)
    for which, full in ((SRC, g.getPoints(SRC)), (TGT, g.getPoints(TGT))):
        kept = g.kept(which)
        _, covs = g.covariances(which)
        if which == SRC:
            V.FastVGICP.setInputSource(o, full[kept, :3])
            o.source_covs = covs
        else:
            V.FastVGICP.setInputTarget(o, full[kept, :3])
            o.target_covs = covs
    return o


# ---------------------------------------------------------------------- the prepared cloud (VC1 .. VC4)
@gpu
@pytest.mark.parametrize("method", (VC.PLANE, VC.MIN_EIG, VC.FROBENIUS), ids=("plane", "min_eig", "frobenius"))
@pytest.mark.parametrize("n", SIZES)
def test_prepared_cloud(vc, reg, pair, prepared, n, method):
    g = _new(vc, reg, regularization=method)
    names = ("source", "target") if n == 2048 else ("target",)
    for name in names:
        which = SRC if name == "source" else TGT
        (g.setInputSource if which == SRC else g.setInputTarget)(pair[name][:n])
        want = prepared(name, n, method)
        kept = g.kept(which)
        assert kept.dtype == np.int32 and np.array_equal(kept, want["kept_index"]), (name, len(kept), len(want["kept_index"]))
        raw, covs = g.covariances(which)
        assert np.array_equal(_bits(raw), _bits(want["raw"]))
        err = np.abs(covs - want["covs"]).max() if len(kept) else 0.0
        big = max(1.0, np.abs(want["covs"]).max()) if len(kept) else 1.0
        print(name, n, method, "kept", len(kept), "regularised covariance error", err, "largest entry", big)
        assert err <= COV_TOL * big
        assert np.array_equal(covs, covs.transpose(0, 2, 1))
        if method != VC.PLANE:
            assert len(kept) == n
    if method == VC.PLANE and n == 20:
        assert len(kept) == 20       # the all-kept case
    if method == VC.PLANE and n == 2048:
        assert 0.5 * n <= len(kept) <= 0.95 * n


@gpu
def test_all_dropped_cloud_and_vc9(vc, reg, pair):
    line = pair["line"]
    for optimizer in (0, 1):
        g = _new(vc, reg, search=2, optimizer=optimizer)
        g.setInputSource(pair["source"][:257])
        g.setInputTarget(line)
        assert len(g.kept(TGT)) == 0 and g.voxel_count() == 0 and len(g.voxels()["counts"]) == 0
        assert g.covariances(TGT)[0].shape == (0, 3, 3)
        c, H, b = g.linearize(np.eye(4))
        assert c == 0.0 and np.all(H == 0.0) and np.all(b == 0.0) and (g.voxel_correspondences() == -1).all()
        guess = pair["guess"]
        T = g.align(guess)
        r = g.result
        assert (r.converged, r.lm_failed, r.n_matched, r.iterations, r.n_linearize, r.n_compute_error) == (0, 0, 0, 0, 1, 0)
        assert np.array_equal(T, guess) and not g.hasConverged()
        # ... and on the source side
        g.swapSourceAndTarget()
        assert len(g.kept(SRC)) == 0 and g.voxel_count() > 0
        c, H, b = g.linearize(np.eye(4))
        assert c == 0.0 and np.all(H == 0.0) and g.voxel_correspondences().shape == (0, 27)
        T = g.align(guess)
        assert (g.result.converged, g.result.n_matched, g.result.n_linearize) == (0, 0, 1) and np.array_equal(T, guess)


@gpu
def test_too_few_points_and_refused_settings(vc, reg, pair):
    g = _new(vc, reg)
    g.setInputTarget(pair["target"][:19])
    with pytest.raises(reg.ApdgicpError) as ei:
        g.kept(TGT)
    assert ei.value.code == -4
    g.setCorrespondenceRandomness(5)          # a no-op (VC1): 19 points are still too few, 20 are enough
    assert g.params.k_correspondences == 20
    with pytest.raises(reg.ApdgicpError):
        g.kept(TGT)
    g.setInputTarget(pair["target"][:20])
    assert len(g.kept(TGT)) == 20
    # a refused setting keeps the last accepted one
    for call, code in ((lambda: g.setNearestNeighborSearchMethod(vc.GPU_RBF_KERNEL), -5), (lambda: g.setRegularizationMethod(vc.NONE), -5),
                       (lambda: g.setRegularizationMethod(vc.NORMALIZED_MIN_EIG), -5), (lambda: g.setNeighborSearchMethod(vc.DIRECT_RADIUS, 4.5), -1),
                       (lambda: g.setNeighborSearchMethod(vc.DIRECT_RADIUS), -1), (lambda: g.setResolution(0.0), -1)):
        with pytest.raises(reg.ApdgicpError) as ei:
            call()
        assert ei.value.code == code
        p, on = g.get_mode()
        assert on and (p.resolution, p.neighbor_search, p.search_radius, p.regularization, p.nn_method) == (1.0, 0, 1.5, vc.PLANE, 0)
    g.setNearestNeighborSearchMethod(vc.GPU_BRUTEFORCE)     # the same exact k-NN
    assert len(g.kept(TGT)) == 20
    g.setKernelWidth(0.3)
    assert (g.kernel_width, g.kernel_max_dist) == (0.3, 1.5)
    for fn in (g.correspondences, g.mahalanobis):
        with pytest.raises(reg.ApdgicpError) as ei:
            fn()
        assert ei.value.code == -5


# ---------------------------------------------------------------------- the map (VC5)
@gpu
@pytest.mark.parametrize("n", (21, 257, 2048))
def test_map_equals_the_vgicp_modes_map_bit_for_bit(vc, vg, reg, pair, n):
    g = _new(vc, reg)
    g.setInputTarget(pair["target"][:n])
    kept = g.kept(TGT)
    _, covs = g.covariances(TGT)
    f = vg.FastVGICP()
    f.setInputTarget(pair["target"][:n][kept])
    f.setTargetCovariances(covs)
    for res in (0.5, 1.0):
        g.setResolution(res)
        f.setResolution(res)
        a, b = g.voxels(), f.voxels()
        assert np.array_equal(a["coords"], b["coords"]) and np.array_equal(a["counts"], b["counts"])
        assert np.array_equal(_bits(a["means"]), _bits(b["means"])) and np.array_equal(_bits(a["covs"]), _bits(b["covs"]))
        assert a["counts"].sum() == len(kept)
        want = V.build_voxelmap(pair["target"][:n][kept], covs, res)
        assert np.array_equal(a["coords"], want["coords"]) and np.array_equal(_bits(a["covs"]), _bits(want["covs"]))
    assert g.build_count() == 2


# ---------------------------------------------------------------------- linearize / compute_error (VC6 .. VC8)
@pytest.fixture(scope="module")
def poses(pair, scene):
    return {"identity": np.eye(4), "guess": pair["guess"].astype(np.float64), "far": scene.make_transform(np.array([2.0, -1.5, 0.3]), 0.2, -0.02, 0.03)}


# (257 offsets per point run through the restatement's Python loop: radius 4 takes the two small block-edge sizes)
LIN_CASES = [(tag, search, radius, n) for tag, search, radius in SEARCHES for n in ((65, 257) if tag == "r4.0" else (20, 65, 257, 2048))]


@gpu
@pytest.mark.parametrize("tag, search, radius, n_src", LIN_CASES, ids=[f"{c[0]}-{c[3]}" for c in LIN_CASES])
def test_linearize_parity(vc, reg, pair, poses, scene, tag, search, radius, n_src):
    g = _new(vc, reg, search=search, radius=radius)
    g.setInputSource(pair["source"][:n_src])
    g.setInputTarget(pair["target"])
    o = _mirror(g)
    assert np.array_equal(g.offsets(), VC.neighbor_offsets(search, radius))
    for name, T in poses.items():
        c, H, b = g.linearize(T)
        corr = g.voxel_correspondences()
        cw, Hw, bw = o.linearize(T)
        assert corr.shape == o.voxel_corr.shape and np.array_equal(corr, o.voxel_corr), name
        if name != "far":
            assert o.n_matched > 0
        if o.n_matched:
            assert rel_err(H, Hw) < HB_TOL and rel_err(b, bw) < HB_TOL and abs(c - cw) <= HB_TOL * cw, (name, rel_err(H, Hw), rel_err(b, bw), abs(c - cw) / cw)
        T1 = scene.make_transform(np.array([0.2, 0.1, 0.0]), 0.01, 0.0, 0.0) @ T
        e, ew = g.compute_error(T1), o.compute_error(T1)
        assert abs(e - ew) <= HB_TOL * max(ew, 1e-300)
        assert np.array_equal(g.voxel_correspondences(), corr)       # compute_error left the frozen indices alone
        # the same bytes on a second run
        c2, H2, b2 = g.linearize(T)
        assert c2 == c and np.array_equal(_bits(H2), _bits(H)) and np.array_equal(_bits(b2), _bits(b)) and np.array_equal(g.voxel_correspondences(), corr)
        assert g.linearize(T, want_Hb=False)[0] == c
    assert g.build_count() == 1
    # n_matched of the record: an align of one iteration linearizes once, at the guess
    g.setMaximumIterations(1)
    g.align(poses["guess"].astype(np.float32))
    o.linearize(poses["guess"].astype(np.float32).astype(np.float64))
    assert g.result.n_linearize == 1 and g.result.n_matched == o.n_matched == int((o.voxel_corr >= 0).sum())


@gpu
def test_direct_radius_one_is_direct7_in_another_order(vc, reg, pair, poses):
    """The two offset lists are equal as sets; the radius loop orders them (-x, -y, -z, 0, +z, +y, +x).  Asserted here: the stored indices
    equal DIRECT7's after that permutation, exactly, and H, b, cost agree to 1e-12 relative (the terms of a point are added in another
    order, so not bit for bit)."""
    a = _new(vc, reg, search=vc.DIRECT7)
    b_ = _new(vc, reg, search=vc.DIRECT_RADIUS, radius=1.0)
    for g in (a, b_):
        g.setInputSource(pair["source"])
        g.setInputTarget(pair["target"])
    o7, o1 = a.offsets().tolist(), b_.offsets().tolist()
    perm = [o7.index(o) for o in o1]
    assert sorted(perm) == list(range(7)) and perm != list(range(7))
    for T in poses.values():
        ca, Ha, ba = a.linearize(T)
        cb, Hb, bb = b_.linearize(T)
        assert np.array_equal(a.voxel_correspondences()[:, perm], b_.voxel_correspondences())
        if ca > 0:
            assert rel_err(Hb, Ha) <= 1e-12 and rel_err(bb, ba) <= 1e-12 and abs(cb - ca) <= 1e-12 * ca


@gpu
@pytest.mark.parametrize("search", (0, 1, 2))
def test_min_eig_equals_the_vgicp_mode_bit_for_bit(vc, vg, reg, pair, poses, search):
    """MIN_EIG filters nothing: a FAST_VGICP handle fed this mode's covariances computes the same H, b and cost, bit for bit."""
    g = _new(vc, reg, search=search, regularization=VC.MIN_EIG)
    g.setInputSource(pair["source"][:700])
    g.setInputTarget(pair["target"])
    assert len(g.kept(SRC)) == 700 and len(g.kept(TGT)) == 2048
    f = vg.FastVGICP()
    f.setNeighborSearchMethod(search)
    f.setInputSource(pair["source"][:700])
    f.setInputTarget(pair["target"])
    f.setSourceCovariances(g.covariances(SRC)[1])
    f.setTargetCovariances(g.covariances(TGT)[1])
    for T in poses.values():
        c, H, b = g.linearize(T)
        cf, Hf, bf = f.linearize(T)
        assert c == cf and np.array_equal(_bits(H), _bits(Hf)) and np.array_equal(_bits(b), _bits(bf))
        assert np.array_equal(g.voxel_correspondences(), f.voxel_correspondences())
        assert g.compute_error(T) == f.compute_error(T)


# ---------------------------------------------------------------------- the loop
# (apdgicp_align_host_loop runs the same function as apdgicp_align in this mode: two searches are enough for the second entry point)
ALIGN_CASES = [(s[0], s[1], s[2], opt, hl) for s in SEARCHES if s[0] in ("d1", "d7", "d27", "r1.5") for opt in (0, 1) for hl in (False, True)
               if not hl or (s[0] in ("d1", "r1.5") and opt == 0)]


@gpu
@pytest.mark.parametrize("tag, search, radius, optimizer, host_loop", ALIGN_CASES,
                         ids=[f"{c[0]}-{'lm' if c[3] == 0 else 'gn'}-{'host_loop' if c[4] else 'align'}" for c in ALIGN_CASES])
def test_align_parity(vc, reg, pair, scene, tag, search, radius, optimizer, host_loop):
    g = _new(vc, reg, search=search, radius=radius, optimizer=optimizer)
    g.setInputSource(pair["source"])
    g.setInputTarget(pair["target"])
    g.setTrace(True)
    guess = pair["guess"]
    T = g.align(guess, host_loop=host_loop)
    o = _mirror(g, optimizer=optimizer)
    To = o.align(guess)
    assert o.face_margin_min >= FACE_MARGIN, o.face_margin_min
    r = g.result
    assert (bool(r.converged), r.iterations, r.n_linearize, r.n_compute_error, r.lm_failed) == (o.converged, o.nr_iterations, o.trace.n_linearize, o.trace.n_compute_error, 0)
    assert r.n_matched == o.n_matched and r.n_matched > 300
    tr = g.trace()
    lm = optimizer == 0
    want = {"lambda": np.array(o.trace.lambdas if lm else []), "rho": np.array(o.trace.rhos if lm else []), "y0": np.array(o.trace.y0s if lm else []),
            "yi": np.array(o.trace.yis if lm else []), "poses": np.array(o.trace.poses).reshape(-1, 4, 4)}
    d = trace_close(tr, want, tol_cost=TRACE_TOL, tol_pose=TRACE_TOL)
    print(tag, "lm" if lm else "gn", "iterations", r.iterations, "trace differences / 1e-11:", d, "face margin", o.face_margin_min)
    assert len(want["poses"]) >= 1 and (not lm or len(want["rho"]) >= 1)
    assert max(d.values()) <= 1.0, d
    te, re_ = scene.pose_error(To, T)
    assert te <= 1e-3 and re_ <= 1e-4
    assert rel_err(g.getFinalHessian(), o.final_hessian) < HB_TOL
    assert np.array_equal(g.voxel_correspondences(), o.voxel_corr)
    # the same bytes on a second run
    rec = bytes(g.result)
    g.align(guess, host_loop=host_loop)
    assert bytes(g.result) == rec


# ---------------------------------------------------------------------- edges (V2 with offsets of magnitude 4)
@gpu
def test_source_coordinates_around_the_key_range_with_radius_4(vc, reg, pair):
    """res 1: a target voxel at cx = 2^20 - 1, the last valid coordinate.  A source point at cx = 2^20 + 3 -- outside the range itself --
    reaches it with the offset (-4, 0, 0); one at 2^20 + 4 reaches nothing; one at 2^20 - 2 has its +2, +3, +4 neighbours outside the range:
    misses, whatever their packed keys would alias."""
    lim = float(1 << 20)
    rng = np.random.default_rng(5)
    far = np.stack([lim + rng.integers(0, 4, size=40) * 0.125, rng.uniform(-0.4, 0.4, size=40), rng.uniform(-0.4, 0.4, size=40)], axis=1).astype(np.float32)
    tgt = np.concatenate([pair["target"][:300], far])
    assert (V.voxel_coord(far[:, 0].astype(np.float64), 1.0) == lim - 1).all()
    src = pair["source"][:300].copy()
    src[7] = (lim + 3.75, 0.1, 0.1)      # c = 2^20 + 3
    src[8] = (lim + 4.75, 0.1, 0.1)      # c = 2^20 + 4
    src[9] = (lim - 1.25, 0.1, 0.1)      # c = 2^20 - 2
    src[10] = (-(lim + 2.25), 0.1, 0.1)  # c = -(2^20 + 3): reaches c = -(2^20 - 1), where nothing is
    assert V.voxel_coord([float(src[7, 0]), float(src[8, 0]), float(src[9, 0]), float(src[10, 0])], 1.0).tolist() == [lim + 3, lim + 4, lim - 2, -(lim + 3)]
    g = _new(vc, reg, search=vc.DIRECT_RADIUS, radius=4.0, regularization=VC.MIN_EIG)   # no filter: every point is a row
    g.setInputSource(src)
    g.setInputTarget(tgt)
    c, H, b = g.linearize(np.eye(4))
    corr = g.voxel_correspondences()
    o = _mirror(g)
    cw, Hw, bw = o.linearize(np.eye(4))
    assert np.array_equal(corr, o.voxel_corr)
    offs = g.offsets().tolist()
    vox = g.voxels()
    v_far = int(np.nonzero((vox["coords"] == [(1 << 20) - 1, -1, -1]).all(axis=1))[0][0])
    assert corr[7, offs.index([-4, 0, 0])] == v_far and (corr[7] >= 0).sum() == 1
    assert (corr[8] == -1).all() and (corr[10] == -1).all()
    assert set(np.nonzero(corr[9] >= 0)[0].tolist()) == {offs.index([1, 0, 0])}
    # (no parity bar on H here: the neighbourhoods of the far points mix coordinates of 1e6 and of 1, their covariances are ill
    # conditioned by construction and cofactors and LU then differ; H, b and cost parity is test_linearize_parity's)
    assert np.isfinite(c) and np.isfinite(H).all() and np.isfinite(b).all() and np.isfinite(cw)


@gpu
def test_refused_target_point_is_named_by_its_original_index(vc, reg, pair):
    """A planar patch at c = 2^20 (the first refused coordinate) appended to the fixture's target: PLANE keeps the patch and has dropped
    points in front of it, so the first refused point's index among the kept points differs from its index in the caller's cloud."""
    lim = float(1 << 20)
    rng = np.random.default_rng(6)
    patch = np.stack([np.full(30, lim + 0.5), rng.uniform(-3, 3, size=30), rng.uniform(-3, 3, size=30)], axis=1).astype(np.float32)
    tgt = np.concatenate([pair["target"], patch])
    g = _new(vc, reg)
    g.setInputTarget(tgt)
    g.setInputSource(pair["source"][:64])
    kept = g.kept(TGT)
    assert 2048 in kept and int(np.nonzero(kept == 2048)[0][0]) < 2048
    for call in (g.voxels, g.voxel_count, lambda: g.linearize(np.eye(4)), g.align):
        with pytest.raises(reg.ApdgicpError) as ei:
            call()
        assert ei.value.code == -1 and "target point 2048 " in str(ei.value), str(ei.value)
    g.setInputTarget(pair["target"])          # the handle stays usable
    assert g.voxel_count() > 0


# ---------------------------------------------------------------------- mode rules (VC10)
@gpu
def test_exclusive_with_the_other_modes(vc, vg, reg, pair):
    ndt = importlib.import_module("riv-slam_amd.ndt")
    icp = importlib.import_module("riv-slam_amd.icp")
    import ctypes as C
    g = _new(vc, reg)
    L = g.L

    def on(getter):
        e = C.c_int()
        reg._check(getter(g.h, None, C.byref(e)))
        return bool(e.value)

    def state():
        return (on(L.apdgicp_get_vgicp_cuda), on(L.apdgicp_get_vgicp), on(L.apdgicp_get_ndt), on(L.apdgicp_get_icp))
    assert state() == (True, False, False, False)
    pv = vg.default_vgicp_params()
    reg._check(L.apdgicp_set_vgicp(g.h, C.byref(pv)))
    assert state() == (False, True, False, False)
    g.enable()
    assert state() == (True, False, False, False)
    pn = ndt.default_ndt_params()
    reg._check(L.apdgicp_set_ndt(g.h, C.byref(pn)))
    assert state() == (False, False, True, False)
    g.enable()
    assert state() == (True, False, False, False)
    pi = icp.default_icp_params()
    reg._check(L.apdgicp_set_icp(g.h, C.byref(pi)))
    assert state() == (False, False, False, True)
    g.enable()
    assert state() == (True, False, False, False)
    g.disable()
    assert state() == (False, False, False, False)
    with pytest.raises(reg.ApdgicpError) as ei:
        g.kept(TGT)
    assert ei.value.code == -3


@gpu
def test_cache_rules(vc, reg, pair, poses):
    src, tgt = pair["source"][:257], pair["target"][:700]
    g = _new(vc, reg)
    g.setInputSource(src, token=11)
    g.setInputTarget(tgt, token=22)
    v0 = g.voxels()
    assert g.build_count() == 1
    g.setInputTarget(tgt.copy(), token=22)         # the same token: no new points
    g.linearize(poses["guess"])
    g.align(poses["guess"].astype(np.float32))
    g.setNeighborSearchMethod(vc.DIRECT_RADIUS, 1.5)   # the offsets are no property of the map
    g.linearize(poses["guess"])
    g.setResolution(1.0)                           # unchanged
    g.setNearestNeighborSearchMethod(vc.GPU_BRUTEFORCE)   # the same k-NN
    g.voxels()
    assert g.build_count() == 1
    g.setResolution(0.5)
    assert g.voxel_count() > len(v0["counts"]) and g.build_count() == 2
    g.setRegularizationMethod(vc.MIN_EIG)          # another prepared cloud: all 700 points
    assert g.voxels()["counts"].sum() == 700 and g.build_count() == 3
    g.setRegularizationMethod(vc.PLANE)
    g.setResolution(1.0)
    v1 = g.voxels()
    assert g.build_count() == 4
    for k in v0:
        assert np.array_equal(v0[k], v1[k])
    kept_s, kept_t = g.kept(SRC), g.kept(TGT)
    g.swapSourceAndTarget()                        # the prepared clouds go with their clouds, the map is the new target's: one rebuild
    assert np.array_equal(g.kept(TGT), kept_s) and np.array_equal(g.kept(SRC), kept_t)
    assert g.voxels()["counts"].sum() == len(kept_s) and g.build_count() == 5
    with pytest.raises(reg.ApdgicpError) as ei:    # the frozen state went with the swap
        g.compute_error(np.eye(4))
    assert ei.value.code == -3
    g.setInputTarget(tgt, token=23)                # new points
    g.voxels()
    assert g.build_count() == 6


@gpu
def test_mode_off_is_a_handle_that_never_had_it_on(vc, reg, pair):
    kw = dict(max_correspondence_distance=2.0, transformation_epsilon=0.01)
    guess = pair["guess"]
    a = reg.FastAPDGICP(reg.default_params(**kw))
    a.setInputSource(pair["source"])
    a.setInputTarget(pair["target"])
    Ta = a.align(guess)
    cov_a = a.getSourceCovariances()
    g = vc.FastVGICPCuda(reg.default_params(**kw))
    g.setInputSource(pair["source"])
    g.setInputTarget(pair["target"])
    g.align(guess)                                  # the mode runs, with covariances of its own
    assert g.result.n_matched > 300
    g.disable()
    Tg = g.align(guess)
    assert bytes(g.result) == bytes(a.result) and np.array_equal(Tg, Ta)
    assert np.array_equal(_bits(g.getSourceCovariances()), _bits(cov_a))
    assert np.array_equal(_bits(g.getFinalHessian()), _bits(a.getFinalHessian()))
