"""Voxelized GICP (fast_gicp::FastVGICP) as a mode of the registration handle: include/apdgicp_hip.h V1 .. V7,
riv-slam_amd/csrc/apd_vgicp.hpp, riv-slam_amd/vgicp.py, against the restatement tests/vgicp_np.py.

CPU part: exports, defaults and self-checks of the restatement.  GPU part (-m gpu): the voxel map bit for bit, linearize /
compute_error / align parity, the cache and mode rules.

Bars: voxel coordinates, counts, order and voxel correspondences exact; fp64 means and covariances of the map bit for bit (the sums
have a stated order, V3); H, b, cost 1e-10 relative and every lambda, rho, cost and pose of an optimiser trace 1e-11 (the project's
bars for the APD path, tests/trace_util.py); final poses 1e-3 m / 1e-4 rad.  The align fixtures are chosen (on the CPU, with the
restatement alone) so that no transformed point comes closer than 1e-9 voxel edges to a voxel face during the whole run -- a
last-bit difference in a pose could otherwise legitimately move a point across a face -- and every test asserts that margin.

One deliberate reading of the issue behind this file: V2 makes a coordinate valid iff |c| < 2^20 with c = floor(x / res - 0.5), so
a point at x = 2^20 res has c = 2^20 - 1 and is VALID; the first invalid coordinates are c = 2^20 (x = (2^20 + 0.5) res) and
c = -2^20 (x = -(2^20 - 0.5) res).  test_v2_* check the rule on both sides of both edges, the point at 2^20 res included.
"""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest

import apdgicp_np as anp
import vgicp_np as V
from conftest import rel_err
from trace_util import trace_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HB_TOL = 1e-10
TRACE_TOL = 1e-11
FACE_MARGIN = 1e-9
LAUNCH = dict(max_correspondence_distance=2.0, transformation_epsilon=0.1)   # reg_transformation_epsilon of the launch file; the gate is ignored (V7)
NEW_SYMBOLS = ("apdgicp_vgicp_default_params", "apdgicp_set_vgicp", "apdgicp_get_vgicp", "apdgicp_vgicp_voxel_count", "apdgicp_vgicp_get_voxels",
               "apdgicp_vgicp_get_correspondences", "apdgicp_vgicp_build_count")


@pytest.fixture(scope="module")
def reg():
    import __graft_entry__ as g
    g.build()
    return importlib.import_module("riv-slam_amd.registration")


@pytest.fixture(scope="module")
def vg(reg):
    return importlib.import_module("riv-slam_amd.vgicp")


# ====================================================================== CPU
def test_new_symbols_are_exported_and_the_module_imports(reg, vg):
    L = reg.load_library()
    header = open(os.path.join(ROOT, "include", "apdgicp_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), f"{name} is not exported"
        assert name in reg.SYMBOLS
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared"
    for name in ("FastVGICP", "VgicpParams", "DIRECT1", "DIRECT7", "DIRECT27", "ADDITIVE", "ADDITIVE_WEIGHTED", "MULTIPLICATIVE"):
        assert hasattr(vg, name)
    for m in ("setResolution", "setNeighborSearchMethod", "setVoxelAccumulationMode", "setInputSource", "setInputTarget", "align", "linearize",
              "compute_error", "voxels", "voxel_correspondences"):
        assert callable(getattr(vg.FastVGICP, m))
    assert issubclass(vg.FastVGICP, reg.FastAPDGICP)
    assert L.apdgicp_abi_version() == 6


def test_default_vgicp_params(vg):
    p = vg.default_vgicp_params()
    assert (p.resolution, p.neighbor_search, p.voxel_mode) == (1.0, vg.DIRECT1, vg.ADDITIVE)   # fast_vgicp_impl.hpp:22-24
    assert ctypes.sizeof(vg.VgicpParams) == 16
    assert (V.DIRECT1, V.DIRECT7, V.DIRECT27) == (vg.DIRECT1, vg.DIRECT7, vg.DIRECT27)


def test_restatement_worked_example_of_the_voxel_coordinate():
    assert V.voxel_coord([0.49, 0.5, 1.5], 1.0).tolist() == [-1.0, 0.0, 1.0]
    assert V.voxel_coord([-0.5], 1.0).tolist() == [-1.0]
    # res 0.5: x / res - 0.5 = 0.48, 0.5, 2.5 and -1.5
    assert V.voxel_coord([0.49, 0.5, 1.5], 0.5).tolist() == [0.0, 0.0, 2.0]
    assert V.voxel_coord([-0.5], 0.5).tolist() == [-2.0]
    pts = np.array([[0.49, 0, 0], [0.5, 0, 0], [1.5, 0, 0]], dtype=np.float32)
    m = V.build_voxelmap(pts, np.tile(np.eye(3), (3, 1, 1)), 1.0)
    assert m["coords"].tolist() == [[-1, -1, -1], [0, -1, -1], [1, -1, -1]] and m["counts"].tolist() == [1, 1, 1]
    assert V.neighbor_offsets(V.DIRECT7).tolist() == [[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]
    o27 = V.neighbor_offsets(V.DIRECT27)
    assert len(o27) == 27 and o27[0].tolist() == [-1, -1, -1] and o27[1].tolist() == [-1, -1, 0] and o27[13].tolist() == [0, 0, 0] and o27[26].tolist() == [1, 1, 1]


def test_restatement_dict_map_equals_the_unique_map():
    rng = np.random.default_rng(11)
    pts = (rng.normal(size=(5000, 3)) * [6, 6, 1.5]).astype(np.float32)
    A = rng.normal(size=(5000, 3, 3))
    covs = A @ A.transpose(0, 2, 1)
    for res in (0.25, 1.0, 3.0):
        a, b = V.build_voxelmap(pts, covs, res), V.build_voxelmap_unique(pts, covs, res)
        assert np.array_equal(a["coords"], b["coords"]) and np.array_equal(a["counts"], b["counts"])
        assert np.array_equal(a["means"].view(np.uint64), b["means"].view(np.uint64))
        assert np.array_equal(a["covs"].view(np.uint64), b["covs"].view(np.uint64))
        assert a["counts"].sum() == 5000 and a["counts"].max() > 1


def _delta(d):
    return anp.FastAPDGICP._delta(np.asarray(d, dtype=np.float64))


def _small_pair(n=400, seed=3):
    rng = np.random.default_rng(seed)
    tgt = (rng.uniform(-1, 1, size=(n, 3)) * [8, 8, 2]).astype(np.float32)
    return tgt


def test_restatement_H_and_b_are_the_derivatives_of_the_frozen_cost():
    """b against first central differences of the frozen cost at a pose with a residual; H against second central differences at
    a pose WITHOUT one (source = target, one point per voxel, identity: e = 0, so the Gauss-Newton H is the whole Hessian).
    cost(delta) = c + 2 b . delta + delta^T H delta + ...; step 1e-6, agreement 1e-5 relative to the largest entry."""
    h = 1e-6
    tgt = _small_pair()
    o = V.FastVGICP(anp.Params(), resolution=1e-3, search=V.DIRECT7)
    o.setInputSource(tgt)
    o.setInputTarget(tgt)
    I = np.eye(4)
    c0, H, b = o.linearize(I)
    assert o.n_matched >= len(tgt) and (o.voxelmap["counts"] == 1).all()
    assert c0 == 0.0 and np.all(b == 0.0)      # the true pose of a noise-free copy, exactly
    Hn = np.zeros((6, 6))
    for i in range(6):
        for j in range(i, 6):
            di, dj = np.eye(6)[i] * h, np.eye(6)[j] * h
            c = [o.compute_error(_delta(si * di + sj * dj)) for si, sj in ((1, 1), (1, -1), (-1, 1), (-1, -1))]
            Hn[i, j] = Hn[j, i] = (c[0] - c[1] - c[2] + c[3]) / (4 * h * h) / 2
    assert np.abs(H - Hn).max() <= 1e-5 * np.abs(H).max(), np.abs(H - Hn).max() / np.abs(H).max()
    # b: a coarser map (several points per voxel) at a pose that leaves a residual
    o = V.FastVGICP(anp.Params(), resolution=1.0, search=V.DIRECT7)
    o.setInputSource(tgt)
    o.setInputTarget(tgt)
    T1 = _delta([0.01, -0.02, 0.015, 0.05, -0.03, 0.02])
    c1, H1, b1 = o.linearize(T1)
    assert c1 > 0 and o.n_matched > len(tgt)
    assert abs(o.compute_error(T1) - c1) <= 1e-12 * c1
    bn = np.array([(o.compute_error(_delta(np.eye(6)[i] * h) @ T1) - o.compute_error(_delta(-np.eye(6)[i] * h) @ T1)) / (4 * h) for i in range(6)])
    assert np.abs(b1 - bn).max() <= 1e-5 * np.abs(b1).max(), np.abs(b1 - bn).max() / np.abs(b1).max()
    assert np.allclose(H1, H1.T, rtol=0, atol=1e-9 * np.abs(H1).max()) and np.linalg.eigvalsh(H1).min() > 0


def test_restatement_cost_vanishes_at_the_true_pose_of_a_noise_free_copy(scene):
    """target = fp32(T source), one point per voxel: e is the fp32 rounding of the target (<= 2^-24 |coordinate| per axis), and
    cost <= n_corr * lambda_max(M) * |e|^2 with lambda_max(M) <= 1 / (2e-3) (PLANE: both covariances have 1e-3 as smallest eigenvalue)."""
    src = _small_pair(300, 5)
    T = scene.make_transform(np.array([0.7, -0.2, 0.05]), 0.05, 0.01, -0.02)
    tgt = (src.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
    o = V.FastVGICP(anp.Params(), resolution=1e-3, search=V.DIRECT1)
    o.setInputSource(src)
    o.setInputTarget(tgt)
    cost, _, _ = o.linearize(T)
    assert o.n_matched > 0.5 * len(src)
    e2 = 3 * (2.0 ** -24 * (np.abs(tgt).max() + 1.0)) ** 2
    assert 0.0 <= cost <= o.n_matched * 500.0 * e2 * 1.01


# ====================================================================== GPU
gpu = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _covs3(c):
    return np.ascontiguousarray(c[:, :3, :3])


def _mirror(g, search=None, res=None, **kw):
    """The restatement with the device's clouds and the DEVICE's covariances (they are tested on their own, 1e-10): what is compared
    here is everything behind them."""
    o = V.FastVGICP(anp.Params(**kw), resolution=g.vparams.resolution if res is None else res, search=g.vparams.neighbor_search if search is None else search)
    o.setInputSource(g.getPoints(0))
    o.setInputTarget(g.getPoints(1))
    o.source_covs = _covs3(g.getSourceCovariances())
    o.target_covs = _covs3(g.getTargetCovariances())
    return o


def _assert_map_equal(got, want):
    assert np.array_equal(got["coords"], want["coords"])
    assert np.array_equal(got["counts"], want["counts"])
    assert np.array_equal(_bits(got["means"]), _bits(want["means"]))
    assert np.array_equal(_bits(got["covs"]), _bits(want["covs"]))


def _scene_cloud(n, seed=21):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(n, 3)) * [7, 7, 1.5]).astype(np.float32)


@gpu
@pytest.mark.parametrize("n", (20, 63, 64, 65, 257, 4099, 65537))  # 65537: 17 radix tiles, the scanned histogram of the pair sort spans two scan tiles
def test_voxel_map_bit_for_bit(vg, n):
    cloud = _scene_cloud(n)
    g = vg.FastVGICP()
    g.setInputTarget(cloud)
    covs = _covs3(g.getTargetCovariances())
    for res in (0.25, 1.0, 3.0):
        g.setResolution(res)
        _assert_map_equal(g.voxels(), V.build_voxelmap(cloud, covs, res))
    assert g.build_count() == 3


def _face_cloud(res):
    """points exactly on voxel faces: x = (m + 0.5) res for positive and negative m (exact in fp32 for res 0.5 and 1.0), mixed with points off them"""
    rng = np.random.default_rng(4)
    m = rng.integers(-9, 10, size=(300, 3))
    on = ((m + 0.5) * res).astype(np.float32)
    off = (rng.uniform(-9, 9, size=(300, 3)) * res).astype(np.float32)
    mixed = on.copy()
    mixed[:, 1:] = off[:, 1:]            # only x on a face
    return np.concatenate([on, off, mixed])[rng.permutation(900)]


SPECIAL = {
    "faces_0.5": lambda: (_face_cloud(0.5), 0.5),
    "faces_1.0": lambda: (_face_cloud(1.0), 1.0),
    "one_voxel": lambda: (_scene_cloud(4099, 8) + np.float32(600.0), 1000.0),
    "own_voxel": lambda: ((np.stack(np.meshgrid(np.arange(9), np.arange(9), np.arange(9), indexing="ij"), -1).reshape(-1, 3)[np.random.default_rng(2).permutation(729)]
                           * 2.0 + 0.25).astype(np.float32), 1.0),
    "duplicates": lambda: (np.repeat(_scene_cloud(130, 9), 3, axis=0)[np.random.default_rng(3).permutation(390)], 1.0),
}


@gpu
@pytest.mark.parametrize("name", sorted(SPECIAL))
def test_voxel_map_special_clouds(vg, name):
    cloud, res = SPECIAL[name]()
    g = vg.FastVGICP()
    g.setResolution(res)
    g.setInputTarget(cloud)
    want = V.build_voxelmap(cloud, _covs3(g.getTargetCovariances()), res)
    got = g.voxels()
    _assert_map_equal(got, want)
    if name == "one_voxel":
        assert len(got["counts"]) == 1 and got["counts"][0] == 4099
    if name == "own_voxel":
        assert (got["counts"] == 1).all() and len(got["counts"]) == 729
    if name.startswith("faces"):
        f = cloud[:, 0].astype(np.float64) / res - 0.5
        assert (f == np.round(f)).sum() >= 600     # the fixture really sits on faces


@gpu
@pytest.mark.parametrize("res", (0.5, 1.0))
def test_v2_target_range(reg, vg, res):
    """|c| < 2^20: c = 2^20 - 1 (x = 2^20 res) and c = -(2^20 - 1) are the last valid coordinates, c = 2^20 and c = -2^20 the first invalid ones"""
    base = _scene_cloud(40, 6)
    lim = float(1 << 20)
    for x, valid, c in ((lim * res, True, (1 << 20) - 1), ((lim + 0.5) * res, False, 1 << 20), (-(lim - 1.5) * res, True, -(1 << 20) + 1), (-(lim - 0.5) * res, False, -(1 << 20))):
        assert float(np.float32(x)) == x and V.voxel_coord([x], res)[0] == c
        for axis in range(3):
            cloud = base.copy()
            cloud[17, axis] = x
            g = vg.FastVGICP(reg.default_params(k_correspondences=5))
            g.setResolution(res)
            g.setInputTarget(cloud)
            g.setInputSource(base)
            if valid:
                got = g.voxels()
                _assert_map_equal(got, V.build_voxelmap(cloud, _covs3(g.getTargetCovariances()), res))
                assert (got["coords"][:, axis] == c).sum() == 1
                g.linearize(np.eye(4))
            else:
                with pytest.raises(reg.ApdgicpError) as ei:
                    g.voxels()
                assert ei.value.code == -1 and "point 17" in str(ei.value)
                with pytest.raises(reg.ApdgicpError) as ei:
                    g.linearize(np.eye(4))
                assert ei.value.code == -1
                with pytest.raises(reg.ApdgicpError) as ei:
                    g.align()
                assert ei.value.code == -1
    cloud = base.copy()
    cloud[3, 1] = np.nan
    g = vg.FastVGICP(reg.default_params(k_correspondences=5))
    g.setInputTarget(cloud)
    with pytest.raises(reg.ApdgicpError):
        g.voxels()


@gpu
@pytest.mark.parametrize("search", (0, 1, 2))
def test_v2_source_points_out_of_range_or_not_finite_are_misses(vg, search):
    rng = np.random.default_rng(12)
    tgt = (rng.normal(size=(3000, 3)) * [3, 3, 1]).astype(np.float32)
    src = (rng.normal(size=(200, 3)) * [2, 2, 0.7]).astype(np.float32)
    A = np.random.default_rng(14).normal(size=(200, 3, 3))
    covs_src = A @ A.transpose(0, 2, 1) + 0.05 * np.eye(3)   # given, not computed: the covariance k-NN wants finite points
    g = vg.FastVGICP()
    g.setNeighborSearchMethod(search)
    g.setInputTarget(tgt)
    g.setInputSource(src)
    g.setSourceCovariances(covs_src)
    T = np.eye(4)
    T[:3, 3] = (0.1, -0.05, 0.02)
    c0, H0, b0 = g.linearize(T)
    corr0 = g.voxel_correspondences()
    bad = src.copy()
    lim = float(1 << 20)
    bad[5] = (lim + 0.5, 0.0, 0.0)         # c = 2^20 at res 1 after the shift by 0.1: out of range
    bad[6] = (0.0, -(lim + 3.0), 0.0)
    bad[7] = (0.0, 0.0, 3.0e38)            # far beyond any int32
    bad[8] = (np.nan, 0.0, 0.0)
    bad[9] = (0.0, np.inf, 0.0)
    bad[10] = (lim - 0.25, 0.0, 0.0)       # c = 2^20 - 1: in range itself, its +x neighbour is not; nothing is there
    assert V.voxel_coord([float(bad[10, 0]) + 0.1], 1.0)[0] == lim - 1 and V.voxel_coord([float(bad[5, 0]) + 0.1], 1.0)[0] == lim
    g.setInputSource(bad)
    g.setSourceCovariances(covs_src)
    c1, H1, b1 = g.linearize(T)
    corr1 = g.voxel_correspondences()
    assert (corr1[5:11] == -1).all()
    keep = np.r_[0:5, 11:200]
    assert np.array_equal(corr1[keep], corr0[keep])
    o = _mirror(g)
    assert np.array_equal(_bits(o.source_covs), _bits(covs_src))
    cw, Hw, bw = o.linearize(T)
    assert np.array_equal(o.voxel_corr, corr1) and o.n_matched > 100
    assert rel_err(H1, Hw) < HB_TOL and rel_err(b1, bw) < HB_TOL and abs(c1 - cw) <= HB_TOL * cw
    assert np.isfinite(c1) and np.isfinite(H1).all()


# ---------------------------------------------------------------------- linearize
@pytest.fixture(scope="module")
def lin_pair(scene):
    src, tgt, T_true, guess = scene.make_pair(2048, 4099, scene.pair_seed(0, 0), "odometry")
    poses = {"identity": np.eye(4), "small": guess.astype(np.float64), "large": scene.make_transform(np.array([3.0, -2.0, 0.4]), 0.3, -0.02, 0.03)}
    return src, tgt, poses


@gpu
@pytest.mark.parametrize("n_src", (20, 64, 65, 257, 2048))
@pytest.mark.parametrize("search", (0, 1, 2))
def test_linearize_parity(vg, lin_pair, search, n_src):
    src, tgt, poses = lin_pair
    g = vg.FastVGICP()
    g.setNeighborSearchMethod(search)
    g.setInputSource(src[:n_src])
    g.setInputTarget(tgt)
    o = _mirror(g)
    for name, T in poses.items():
        c, H, b = g.linearize(T)
        cw, Hw, bw = o.linearize(T)
        assert np.array_equal(g.voxel_correspondences(), o.voxel_corr), name
        assert o.n_matched > 0
        assert rel_err(H, Hw) < HB_TOL and rel_err(b, bw) < HB_TOL and abs(c - cw) <= HB_TOL * cw, (name, rel_err(H, Hw), rel_err(b, bw), abs(c - cw) / cw)
        c2, _, _ = g.linearize(T, want_Hb=False)
        assert c2 == c
    assert g.build_count() == 1


@gpu
@pytest.mark.parametrize("optimizer", (0, 1))
def test_source_outside_the_map_and_v7(reg, vg, lin_pair, optimizer):
    src, tgt, _ = lin_pair
    g = vg.FastVGICP(reg.default_params(optimizer=optimizer))
    g.setNeighborSearchMethod(vg.DIRECT27)
    g.setInputSource(src[:257] + np.float32(5000.0))
    g.setInputTarget(tgt)
    c, H, b = g.linearize(np.eye(4))
    assert c == 0.0 and np.all(H == 0.0) and np.all(b == 0.0) and (g.voxel_correspondences() == -1).all()
    guess = np.eye(4, dtype=np.float32)
    guess[:3, 3] = (0.5, 0.25, -0.125)
    T = g.align(guess)
    r = g.result
    assert (r.converged, r.lm_failed, r.n_matched, r.iterations, r.n_linearize, r.n_compute_error) == (0, 0, 0, 0, 1, 0)
    assert not g.hasConverged() and np.array_equal(T, guess) and r.final_cost == 0.0
    o = _mirror(g, **dict(optimizer=optimizer))
    assert np.array_equal(o.align(guess), guess) and not o.converged and o.n_matched == 0


# ---------------------------------------------------------------------- compute_error
@gpu
@pytest.mark.parametrize("search", (0, 1))
def test_compute_error_uses_the_frozen_state(vg, scene, lin_pair, search):
    src, tgt, poses = lin_pair
    g = vg.FastVGICP()
    g.setNeighborSearchMethod(search)
    g.setInputSource(src)
    g.setInputTarget(tgt)
    o = _mirror(g)
    T0 = poses["small"]
    T1 = scene.make_transform(np.array([0.4, 0.3, 0.0]), 0.02, 0.0, 0.0) @ T0
    # the precondition, on the CPU: linearizing at T1 changes the correspondences and the cost
    p = _mirror(g)
    c_T1, _, _ = p.linearize(T1)
    corr_T1 = p.voxel_corr.copy()
    cw0, _, _ = o.linearize(T0)
    assert (corr_T1 != o.voxel_corr).sum() > 100
    frozen = o.compute_error(T1)
    assert abs(frozen - c_T1) > 1e-3 * c_T1
    c0, _, _ = g.linearize(T0)
    e1 = g.compute_error(T1)
    assert abs(c0 - cw0) <= HB_TOL * cw0
    assert abs(e1 - frozen) <= HB_TOL * frozen, abs(e1 - frozen) / frozen
    assert abs(g.compute_error(T0) - cw0) <= HB_TOL * cw0
    assert np.array_equal(g.voxel_correspondences(), o.voxel_corr)     # compute_error left them alone
    c1, _, _ = g.linearize(T1)
    assert abs(c1 - c_T1) <= HB_TOL * c_T1 and abs(c1 - e1) > 1e-3 * c1


# ---------------------------------------------------------------------- align
# (name, parameters, search, resolution, pair seed index): chosen on the CPU with the restatement alone (face margin of the whole run >= 1e-9)
ALIGN_CASES = (
    ("launch_d1", LAUNCH, 0, 1.0, 0),
    ("launch_d7", LAUNCH, 1, 1.0, 1),
    ("default_d1", {}, 0, 1.0, 2),
    ("default_d7", {}, 1, 1.0, 7),
    ("plane_d7_res2", dict(regularization=3, transformation_epsilon=0.01), 1, 2.0, 4),
    ("frobenius_d1", dict(regularization=4, transformation_epsilon=0.01), 0, 1.0, 5),
)


def _align_case(scene, name):
    tag, kw, search, res, idx = next(c for c in ALIGN_CASES if c[0] == name)
    src, tgt, T_true, guess = scene.make_pair(2048, 4099, scene.pair_seed(7, idx), "odometry")
    return kw, search, res, src, tgt, guess


def test_align_fixtures_keep_their_distance_from_the_voxel_faces(scene):
    """The condition of the align parity tests, checked where the fixtures are chosen: on the CPU, with the restatement alone (its own
    covariances), one LM run per scene -- the GPU tests assert the margin of their own run again."""
    for name, kw, search, res, idx in ALIGN_CASES:
        kw_, search_, res_, src, tgt, guess = _align_case(scene, name)
        o = V.FastVGICP(anp.Params(**kw), resolution=res, search=search)
        o.setInputSource(src)
        o.setInputTarget(tgt)
        o.align(guess)
        assert o.face_margin_min >= FACE_MARGIN and o.n_matched > 500


def _align_parity(reg, vg, scene, name, optimizer, host_loop):
    kw, search, res, src, tgt, guess = _align_case(scene, name)
    kw = dict(kw, optimizer=optimizer)
    g = vg.FastVGICP(reg.default_params(**kw))
    g.setResolution(res)
    g.setNeighborSearchMethod(search)
    g.setInputSource(src)
    g.setInputTarget(tgt)
    g.setTrace(True)
    T = g.align(guess, host_loop=host_loop)
    o = _mirror(g, **kw)
    To = o.align(guess)
    assert o.face_margin_min >= FACE_MARGIN, o.face_margin_min
    r = g.result
    assert (bool(r.converged), r.iterations, r.n_linearize, r.n_compute_error, r.lm_failed) == (o.converged, o.nr_iterations, o.trace.n_linearize, o.trace.n_compute_error, 0)
    assert r.n_matched == o.n_matched and r.n_matched > 500
    tr = g.trace()
    lm = optimizer == 0
    want = {"lambda": np.array(o.trace.lambdas if lm else []), "rho": np.array(o.trace.rhos if lm else []), "y0": np.array(o.trace.y0s if lm else []),
            "yi": np.array(o.trace.yis if lm else []), "poses": np.array(o.trace.poses).reshape(-1, 4, 4)}
    d = trace_close(tr, want, tol_cost=TRACE_TOL, tol_pose=TRACE_TOL)
    print(name, "lm" if lm else "gn", "iterations", r.iterations, "trace differences / 1e-11:", d, "face margin", o.face_margin_min)
    assert len(want["poses"]) >= 1 and (not lm or len(want["rho"]) >= 1)
    assert max(d.values()) <= 1.0, d
    te, re_ = scene.pose_error(To, T)
    assert te <= 1e-3 and re_ <= 1e-4
    assert rel_err(g.getFinalHessian(), o.final_hessian) < HB_TOL
    assert np.array_equal(g.voxel_correspondences(), o.voxel_corr)


@gpu
@pytest.mark.parametrize("optimizer", (0, 1), ids=("lm", "gn"))
@pytest.mark.parametrize("name", [c[0] for c in ALIGN_CASES])
def test_align_parity(reg, vg, scene, name, optimizer):
    _align_parity(reg, vg, scene, name, optimizer, False)


@gpu
@pytest.mark.parametrize("name", ("launch_d1", "default_d7"))
def test_align_host_loop_entry_point_runs_the_same_loop(reg, vg, scene, name):
    _align_parity(reg, vg, scene, name, 0, True)


# ---------------------------------------------------------------------- cache and mode rules
@gpu
def test_cache_rules(reg, vg, lin_pair):
    src, tgt, poses = lin_pair
    src, tgt = src[:257], tgt[:700]
    g = vg.FastVGICP()
    g.setInputSource(src, token=11)
    g.setInputTarget(tgt, token=22)
    v0 = g.voxels()
    assert g.build_count() == 1
    g.setInputTarget(tgt.copy(), token=22)       # the same token: the reference's pointer-equality early return
    g.linearize(poses["small"])
    g.align(poses["small"])
    g.setNeighborSearchMethod(vg.DIRECT7)        # the search method is no property of the map
    g.linearize(poses["small"])
    g.setResolution(1.0)                         # unchanged
    v1 = g.voxels()
    assert g.build_count() == 1
    _assert_map_equal(v1, v0)
    g.setResolution(0.5)
    assert len(g.voxels()["counts"]) > len(v0["counts"]) and g.build_count() == 2
    g.setResolution(1.0)
    _assert_map_equal(g.voxels(), v0)
    assert g.build_count() == 3
    covs = g.getTargetCovariances()
    g.setTargetCovariances(covs * 2.0)           # set_covariances(TARGET)
    v2 = g.voxels()
    assert g.build_count() == 4
    assert np.array_equal(v2["coords"], v0["coords"]) and np.array_equal(_bits(v2["covs"]), _bits(v0["covs"] * 2.0)) and np.array_equal(_bits(v2["means"]), _bits(v0["means"]))
    g.setSourceCovariances(g.getSourceCovariances())   # the source's covariances are none of the map's business
    g.voxels()
    assert g.build_count() == 4
    g.swapSourceAndTarget()
    v3 = g.voxels()
    assert g.build_count() == 5
    _assert_map_equal(v3, V.build_voxelmap(src, _covs3(g.getTargetCovariances()), 1.0))
    with pytest.raises(reg.ApdgicpError) as ei:
        g.compute_error(poses["small"])          # the frozen state went with the swap
    assert ei.value.code == -3
    g.setInputTarget(tgt, token=23)              # another token
    g.voxels()
    assert g.build_count() == 6
    g.setCorrespondenceRandomness(10)            # invalidates the covariances, hence the map
    g.linearize(poses["small"])
    assert g.build_count() == 7
    g.clearTarget()
    with pytest.raises(reg.ApdgicpError):
        g.voxels()


@gpu
def test_mode_rules_and_the_apd_path_is_left_alone(reg, vg, scene):
    src, tgt, _, guess = scene.make_pair(2048, 2048, scene.pair_seed(0, 0), "odometry")
    kw = dict(max_correspondence_distance=2.0, transformation_epsilon=0.01, azimuth_variance_deg=1.0)
    fresh = reg.FastAPDGICP(reg.default_params(**kw))
    fresh.setInputSource(src)
    fresh.setInputTarget(tgt)
    fresh.align(guess)
    want = bytes(fresh.result)
    want_corr = fresh.correspondences()
    g = vg.FastVGICP(reg.default_params(**kw))
    assert g.enabled()
    g.setInputSource(src)
    g.setInputTarget(tgt)
    with pytest.raises(reg.ApdgicpError) as ei:
        g.setVoxelAccumulationMode(vg.MULTIPLICATIVE)
    assert ei.value.code == -5 and g.vparams.voxel_mode == vg.ADDITIVE
    g.setVoxelAccumulationMode(vg.ADDITIVE_WEIGHTED)      # the same branch as ADDITIVE (fast_vgicp_voxel.hpp:138-141)
    with pytest.raises(reg.ApdgicpError) as ei:
        g.setResolution(0.0)
    assert ei.value.code == -1
    with pytest.raises(reg.ApdgicpError) as ei:
        g.setNeighborSearchMethod(3)
    assert ei.value.code == -1
    g.align(guess)
    assert bytes(g.result) != want
    for call in (g.correspondences, g.mahalanobis):
        with pytest.raises(reg.ApdgicpError) as ei:
            call()
        assert ei.value.code == -5
    # what does not depend on the cost keeps working
    assert g.getFitnessScore(T=guess) == fresh.getFitnessScore(T=guess)
    assert np.array_equal(g.nearestNeighbours(guess)[0], fresh.nearestNeighbours(guess)[0])
    assert np.array_equal(g.transformSource(guess), fresh.transformSource(guess)) and np.array_equal(g.getPoints(0), src)
    g.disable()                                            # apdgicp_set_vgicp(h, NULL)
    assert not g.enabled()
    with pytest.raises(reg.ApdgicpError):
        g.voxels()
    g.align(guess)
    assert bytes(g.result) == want
    got_corr = g.correspondences()
    assert np.array_equal(got_corr[0], want_corr[0]) and np.array_equal(got_corr[1].view(np.uint32), want_corr[1].view(np.uint32))
    g.enable()
    g.align(guess)
    assert bytes(g.result) != want and g.build_count() == 1


# ---------------------------------------------------------------------- nothing stale: clouds and covariances replaced through OTHER entry points
def _assert_linearize_equals_mirror(g, T):
    c, H, b = g.linearize(T)
    o = _mirror(g)
    cw, Hw, bw = o.linearize(T)
    assert o.n_matched > 0 and np.array_equal(g.voxel_correspondences(), o.voxel_corr)
    assert rel_err(H, Hw) < HB_TOL and rel_err(b, bw) < HB_TOL and abs(c - cw) <= HB_TOL * cw, (rel_err(H, Hw), rel_err(b, bw), abs(c - cw) / cw)
    e = g.compute_error(T)
    assert abs(e - cw) <= HB_TOL * cw


@gpu
@pytest.mark.parametrize("between", ("fitness", "nearest", "inlier", "mode_off_align", "mode_off_linearize"))
@pytest.mark.parametrize("change", ("set_source", "swap"))
def test_a_new_and_larger_source_is_never_read_through_the_old_permutation(reg, vg, lin_pair, change, between):
    """The source is replaced by a LARGER one (set_source, or swap with a larger target) after a linearize, and a call that is not a
    voxelized linearize -- fitness score, nearest neighbours, inlier fraction, an APD-GICP align or linearize with the mode off --
    sets the pair up again before the next voxelized linearize: that one must use the new source's own covariances, point by point."""
    src, tgt, poses = lin_pair
    T = poses["small"]
    g = vg.FastVGICP()
    g.setNeighborSearchMethod(vg.DIRECT7)
    g.setInputSource(src[:257])
    g.setInputTarget(tgt[:1500] if change == "swap" else tgt)
    _assert_linearize_equals_mirror(g, T)
    if change == "set_source":
        g.setInputSource(src)                      # 2 048 > 257 points
        Tn = T
    else:
        g.swapSourceAndTarget()                    # the source is now the 1 500-point cloud
        Tn = np.linalg.inv(T)
    with pytest.raises(reg.ApdgicpError) as ei:
        g.compute_error(Tn)                        # the frozen state belonged to the old source
    assert ei.value.code == -3
    if between == "fitness":
        g.getFitnessScore(T=Tn.astype(np.float32))
    elif between == "nearest":
        g.nearestNeighbours(Tn.astype(np.float32))
    elif between == "inlier":
        g.inlierFraction(0.5, T=Tn.astype(np.float32))
    else:
        g.disable()
        if between == "mode_off_align":
            g.align(Tn.astype(np.float32))
        else:
            reg.FastAPDGICP.linearize(g, Tn)
        g.enable()
    with pytest.raises(reg.ApdgicpError) as ei:
        g.compute_error(Tn)
    assert ei.value.code == -3
    assert g.n_src == (2048 if change == "set_source" else 1500)
    _assert_linearize_equals_mirror(g, Tn)
    r = g.align(Tn.astype(np.float32))
    assert g.result.n_matched > 0 and np.isfinite(r).all()


@gpu
@pytest.mark.parametrize("route", ("get_covariances", "compute_covariances", "fitness", "nearest", "mode_off_align"))
def test_the_map_follows_recomputed_target_covariances(reg, vg, lin_pair, route):
    """A parameter change invalidates the covariances; whichever call recomputes them, the map served afterwards is built from the NEW ones
    (= what get_covariances returns), and one rebuild is all it takes."""
    src, tgt, poses = lin_pair
    src, tgt = src[:257], tgt[:1500]
    T = poses["small"].astype(np.float32)
    g = vg.FastVGICP()
    g.setInputSource(src)
    g.setInputTarget(tgt)
    v0 = g.voxels()
    g.linearize(poses["small"])
    assert g.build_count() == 1
    for step, change in enumerate((lambda: g.setCorrespondenceRandomness(10), lambda: g.setRegularizationMethod(reg.REG_FROBENIUS))):
        change()
        if route == "get_covariances":
            g.getTargetCovariances()
        elif route == "compute_covariances":
            g.computeCovariances(reg.TARGET)
        elif route == "fitness":
            g.getFitnessScore(T=T)
        elif route == "nearest":
            g.nearestNeighbours(T)
        else:
            g.disable()
            g.align(T)
            g.enable()
        with pytest.raises(reg.ApdgicpError) as ei:
            g.compute_error(poses["small"])        # frozen against the old map and the old source covariances
        assert ei.value.code == -3
        got = g.voxels()
        want = V.build_voxelmap(tgt, _covs3(g.getTargetCovariances()), 1.0)
        _assert_map_equal(got, want)
        assert not np.array_equal(_bits(got["covs"]), _bits(v0["covs"]))
        assert g.build_count() == 2 + step
        _assert_linearize_equals_mirror(g, poses["small"])
        assert g.build_count() == 2 + step
        v0 = got
