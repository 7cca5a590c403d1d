"""Map cloud generation on the device (riv-slam_amd/map_cloud.py, csrc/apd_map.hpp) against radar_graph_slam::MapCloudGenerator::generate
(radar_graph_slam/src/radar_graph_slam/map_cloud_generator.cpp:13-53).

The expected values come from tests/map_cloud_np.py, a numpy restatement of include/apdgicp_hip.h's "map cloud generation" section (M1 .. M6).
Every comparison is bit for bit: the pushed fp32 coordinates, the counts, the depth, min / max as fp64 bits, the number and order of the
output points, the centres as fp32 bits.  The one exception is the payload of a NaN, which IEEE 754 leaves open: a NaN coordinate has to
be a NaN coordinate, whatever its bits.
"""
import importlib
import os

import numpy as np
import pytest

import map_cloud_np as mnp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
NEW_SYMBOLS = ["apdgicp_map_cloud_create", "apdgicp_map_cloud_destroy", "apdgicp_map_cloud_add_keyframe", "apdgicp_map_cloud_clear", "apdgicp_map_cloud_generate",
               "apdgicp_map_cloud_points", "apdgicp_map_cloud_copy", "apdgicp_map_cloud_info"]
I4 = np.eye(4)


def cloud(rng, n, sigma=(12.0, 12.0, 1.5), beyond=0):
    """n points inside the 50 m gate (+ `beyond` points past it, spread through the cloud), with an intensity column"""
    c = np.zeros((n + beyond, 4), dtype=F32)
    p = rng.normal(size=(n, 3)) * sigma
    r = np.linalg.norm(p, axis=1)
    p[r > 45.0] *= (45.0 / r[r > 45.0])[:, None]
    far = np.zeros(n + beyond, dtype=bool)
    far[rng.choice(n + beyond, beyond, replace=False)] = True
    c[~far, :3] = p
    c[far, :3] = rng.uniform(60.0, 90.0, (beyond, 1)) * [1.0, 0.0, 0.0]
    c[:, 3] = rng.uniform(0.0, 60.0, n + beyond)
    return c


def pose(scene, rng, far=300.0):
    """a non-trivial rotation and a translation of a few hundred metres"""
    return scene.make_transform(rng.uniform(-far, far, 3) * [1.0, 1.0, 0.02], rng.uniform(-3.0, 3.0), rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1))


def same_f32(a, b):
    a, b = np.ascontiguousarray(a, dtype=F32), np.ascontiguousarray(b, dtype=F32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def same_f64(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float64).view(np.uint64), np.ascontiguousarray(b, dtype=np.float64).view(np.uint64))


# ---------------------------------------------------------------------------------------------------------------- the restatement (no GPU)
def test_worked_example_in_both_orders():
    a = np.array([[0, 0, 0], [1.5, 0, 0]], dtype=F32)
    r = mnp.generate([a], [I4], 1.0)
    assert r["depth"] == 2 and r["rounds"] == 1
    assert np.array_equal(r["min"], [-1.0, -3.0, -3.0]) and np.array_equal(r["max"], np.array([-1.0, -3.0, -3.0]) + (4.0 - mnp.EPS))
    assert np.array_equal(mnp.keys_of(r["pushed"], r["min"], 1.0), [[1, 3, 3], [2, 3, 3]])
    assert np.array_equal(r["points"], [[0.5, 0.5, 0.5, 0], [1.5, 0.5, 0.5, 0]])
    s = mnp.generate([a[::-1]], [I4], 1.0)   # the grid origin depends on the order of arrival: a min / max-anchored grid gets this one wrong
    assert np.array_equal(s["min"], [-1.5, -3.0, -3.0]) and s["depth"] == 2
    assert np.array_equal(s["points"], [[0.0, 0.5, 0.5, 0], [2.0, 0.5, 0.5, 0]])


@pytest.mark.parametrize("n", [1, 2, 65, 5000])
def test_sequential_box_equals_first_violator_per_round(n):
    rng = np.random.default_rng(100 + n)
    for res in (0.05, 0.3, 1.0):
        p = np.zeros((n, 4), dtype=F32)
        p[:, :3] = rng.normal(size=(n, 3)) * [300.0, 300.0, 5.0]
        if n > 2:
            p[rng.integers(1, n), 0] = np.nan
        s, q = mnp.box_seq(p, res), mnp.box_rounds(p, res)
        assert same_f64(s[0], q[0]) and same_f64(s[1], q[1]) and s[2:] == q[2:]


def test_every_point_lies_in_exactly_one_output_voxel_and_keys_ascend(scene):
    rng = np.random.default_rng(7)
    clouds = [cloud(rng, n, beyond=3) for n in (900, 0, 1300)]
    poses = [pose(scene, rng) for _ in clouds]
    for res in (0.05, 0.3, 1.0):
        r = mnp.generate(clouds, poses, res)
        assert r["n_pushed"] == 2200 and r["n_out"] == len(r["keys"]) and (np.diff(r["keys"].astype(np.int64)) > 0).all()
        p = r["pushed"][mnp.finite_rows(r["pushed"]), :3].astype(np.float64)
        c = r["points"][:, :3].astype(np.float64)
        slack = res / 2 + np.spacing(np.abs(r["points"][:, :3]).max())   # (the centre is rounded to fp32)
        k = mnp.keys_of(r["pushed"], r["min"], res)
        own = np.searchsorted(r["keys"], mnp.interleave(k, r["depth"]))
        assert (np.abs(p - c[own]) <= slack).all()
        assert len(np.unique(r["points"][:, :3], axis=0)) == r["n_out"]   # distinct voxels have distinct centres: no second one can hold the point


def test_the_library_exports_the_new_symbols():
    import __graft_entry__ as g
    g.build()
    reg = importlib.import_module("riv-slam_amd.registration")
    L = reg.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name) and name in reg.SYMBOLS
    assert L.apdgicp_abi_version() == 6


# ---------------------------------------------------------------------------------------------------------------- the device
@pytest.fixture(scope="module")
def mods():
    import __graft_entry__ as g
    g.build()
    return importlib.import_module("riv-slam_amd.registration"), importlib.import_module("riv-slam_amd.map_cloud")


def fresh(mods, clouds, **kw):
    g = mods[1].MapCloudGenerator()
    for q, c in enumerate(clouds):
        assert g.add_keyframe(c, **kw) == q
    return g


def assert_equals(g, want, pts=None):
    """the last generate of g against the restatement's dict"""
    info = g.info()
    pts = g.to_numpy() if pts is None else pts
    for k in ("n_input", "n_pushed", "n_finite", "n_out", "depth", "rounds"):
        assert info[k] == want[k], (k, info[k], want[k])
    assert same_f64(info["min"], want["min"]) and same_f64(info["max"], want["max"])
    assert g.n == want["n_out"] and same_f32(pts, want["points"])


def run_and_check(mods, clouds, poses, res, ids=None, linear=False, g=None):
    """pushed cloud (res = 0) and octree output of a generator against the restatement; returns the restatement's octree dict"""
    g = g or fresh(mods, clouds)
    ids = list(range(len(clouds))) if ids is None else ids
    visited = [clouds[i] for i in ids]
    g.generate(poses, ids, 0.0, linear)
    assert_equals(g, mnp.generate(visited, poses, 0.0, linear))
    g.generate(poses, ids, res, linear)
    want = mnp.generate(visited, poses, res, linear)
    assert_equals(g, want)
    return want


@pytest.mark.gpu
def test_gpu_worked_example_in_both_orders(mods):
    a = np.array([[0, 0, 0, 5], [1.5, 0, 0, 6]], dtype=F32)
    g = fresh(mods, [a, a[::-1].copy()])
    assert g.generate([I4], [0], 1.0) == 2
    assert np.array_equal(g.to_numpy(), [[0.5, 0.5, 0.5, 0], [1.5, 0.5, 0.5, 0]])
    i = g.info()
    assert np.array_equal(i["min"], [-1.0, -3.0, -3.0]) and same_f64(i["max"], np.array([-1.0, -3.0, -3.0]) + (4.0 - mnp.EPS)) and i["depth"] == 2 and i["rounds"] == 1
    assert g.generate([I4], [1], 1.0) == 2   # the other order: another origin, other centres
    assert np.array_equal(g.to_numpy(), [[0.0, 0.5, 0.5, 0], [2.0, 0.5, 0.5, 0]]) and np.array_equal(g.info()["min"], [-1.5, -3.0, -3.0])


def split(c, k):
    """the cloud over k keyframes of unequal sizes: k = 3 with an empty one first, k = 7 with an empty one in the middle and one last"""
    n = len(c)
    if k == 1:
        return [c]
    if k == 3:
        cut = [0, 0, n // 3, n]
    else:
        cut = [0, n // 11, n // 5, n // 5, n // 2, (3 * n) // 4, n, n]
    return [np.ascontiguousarray(c[cut[q]:cut[q + 1]]) for q in range(k)]


# launch shapes: one point per lane in blocks of 1024 (gate, push, keys, heads); 4096 points per block of the box search; radix tiles and scan
# tiles of 4096; the scanned histogram has 256 entries per radix tile, so above 16 tiles (65 536 keys) it spans a second scan tile
@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 65537])
def test_gpu_sizes_at_the_edges_of_the_launch_shapes(mods, scene, n):
    rng = np.random.default_rng(1000 + n)
    c = cloud(rng, n, beyond=5)   # n pushed points
    for k in (1, 3, 7):
        parts = split(c, k)
        poses = [pose(scene, rng, 100.0) for _ in parts]
        want = run_and_check(mods, parts, poses, 0.05 if k != 3 else 0.3)
        assert want["n_pushed"] == n and want["n_input"] == n + 5


@pytest.mark.gpu
def test_gpu_gate_exactness_and_non_finite_points(mods):
    """The gate is d > 50 on the fp32 norm.  Candidates around 50 on the x axis and (30, 40, 0) (norm exactly 50): the three norms
    nextafter(50, -inf), 50 and nextafter(50, +inf) all occur; the first two are kept.  A NaN input coordinate is kept (its norm is NaN);
    an infinite INPUT coordinate has the norm +inf and is gated out; a pushed coordinate becomes +-inf where the fp32 product overflows.
    The non-finite pushed points are in the res <= 0 output and not in the octree."""
    f50 = F32(50.0)
    lo, hi = np.nextafter(f50, F32(-np.inf)), np.nextafter(f50, F32(np.inf))
    xs = f50 + np.arange(-8, 9).astype(F32) * np.spacing(f50)
    cand = np.zeros((len(xs) + 1, 4), dtype=F32)
    cand[:-1, 0], cand[-1, :3] = xs, (30.0, 40.0, 0.0)
    norms = np.sqrt((cand[:, 0] * cand[:, 0] + cand[:, 1] * cand[:, 1]) + cand[:, 2] * cand[:, 2])
    assert {lo, f50, hi} <= set(norms.tolist()) and norms[-1] == f50
    cand[:, 3] = np.arange(len(cand))
    g = fresh(mods, [cand])
    g.generate([I4], None, 0.0)
    kept = g.to_numpy()
    assert np.array_equal(kept[:, 3], cand[norms <= f50, 3]) and (norms == hi).any()
    assert_equals(g, mnp.generate([cand], [I4], 0.0), kept)
    odd = np.array([[1, 2, 0, 1], [np.nan, 0, 0, 2], [np.inf, 0, 0, 3], [0, -np.inf, 0, 4], [5, 0, 10, 5], [0, 4, np.nan, 6], [-5, 2, -10, 7], [3, 3, 0, 8]], dtype=F32)
    P = np.eye(4)
    P[0, 2] = 1e38   # x' = x + 1e38 z: +-inf in fp32 for z = +-10, x for z = 0
    for linear in (False, True):
        g = fresh(mods, [odd])
        g.generate([P], None, 0.0, linear)
        out = g.to_numpy()
        assert np.array_equal(out[:, 3], [1, 2, 5, 6, 7, 8]) and out[2, 0] == np.inf and out[4, 0] == -np.inf and np.isnan(out[1, 0]) and np.isnan(out[3, 2])
        assert_equals(g, mnp.generate([odd], [P], 0.0, linear), out)
        g.generate([P], None, 0.5, linear)
        want = mnp.generate([odd], [P], 0.5, linear)
        assert want["n_pushed"] == 6 and want["n_finite"] == 2 and np.isfinite(g.to_numpy()).all()
        assert_equals(g, want)
    g = fresh(mods, [odd[1:4]])   # nothing finite: an empty map, status 0
    assert g.generate([I4], None, 0.05) == 0 and g.info()["n_pushed"] == 1 and g.info()["n_finite"] == 0 and g.points().n == 0


@pytest.mark.gpu
@pytest.mark.parametrize("res", [1.0, 0.05])
def test_gpu_points_on_the_box_faces(mods, res):
    """after a base cloud, ONE more point on min[a], on max[a] (both rounded to fp32) or one fp32 ulp either side of them: on or above
    min and below max the box stays, otherwise it grows exactly as the sequential loop says.  res = 1: the box is dyadic, min[a] is an fp32
    number (on it: no growth) and max[a] = min[a] + 2^depth - eps rounds up to an fp32 number >= max[a] (on it: growth)."""
    rng = np.random.default_rng(11)
    base = np.zeros((300, 4), dtype=F32)
    base[1:, :3] = rng.normal(size=(299, 3)) * [1.5, 1.2, 0.4]
    b = mnp.generate([base], [I4], res)
    extra = []
    for a in range(3):
        for edge in (F32(b["min"][a]), F32(b["max"][a])):
            for v in (np.nextafter(edge, F32(-np.inf)), edge, np.nextafter(edge, F32(np.inf))):
                p = np.zeros((1, 4), dtype=F32)
                p[0, a] = v
                extra.append(p)
    g = fresh(mods, [base] + extra)
    grew = []
    for q in range(len(extra)):
        g.generate([I4, I4], [0, 1 + q], res)
        want = mnp.generate([base, extra[q]], [I4, I4], res)
        assert_equals(g, want)
        grew.append(want["rounds"] - b["rounds"])
    assert set(grew) == {0, 1}
    if res == 1.0:
        assert grew == [1, 0, 0, 0, 1, 1] * 3


@pytest.mark.gpu
def test_gpu_first_finite_point_after_leading_nan_points(mods, scene):
    rng = np.random.default_rng(12)
    c = cloud(rng, 500)
    c[:70, 1] = np.nan   # more than one wave of them
    c[200, 2] = np.nan
    want = run_and_check(mods, [c], [pose(scene, rng)], 0.1)
    assert want["n_finite"] == 429 and want["n_pushed"] == 500


@pytest.mark.gpu
@pytest.mark.parametrize("res", [0.05, 0.1, 1.0])
def test_gpu_points_on_voxel_faces(mods, res):
    """min + k * res rounded to fp32 and its two neighbours, on every axis: the key is the truncated IEEE quotient"""
    rng = np.random.default_rng(13)
    base = cloud(rng, 400, sigma=(8.0, 8.0, 1.0))
    b = mnp.generate([base], [I4], res)
    ks = rng.integers(1, (1 << b["depth"]) - 1, 200)
    face = np.zeros((3 * 3 * len(ks), 4), dtype=F32)
    row = 0
    for a in range(3):
        f = (b["min"][a] + ks * res).astype(F32)
        for v in (np.nextafter(f, F32(-np.inf)), f, np.nextafter(f, F32(np.inf))):
            inside = (np.abs(v) < 35.0)   # (the gate)
            face[row:row + len(ks), a] = np.where(inside, v, 0)
            row += len(ks)
    want = run_and_check(mods, [base, face], [I4, I4], res)
    assert want["rounds"] == b["rounds"] and same_f64(want["min"], b["min"])   # all inside: the grid is the base cloud's


@pytest.mark.gpu
def test_gpu_both_product_orders(mods, scene):
    rng = np.random.default_rng(14)
    clouds = [cloud(rng, n, beyond=2) for n in (3000, 2500)]
    poses = [pose(scene, rng) for _ in clouds]
    a = run_and_check(mods, clouds, poses, 0.05, linear=False)
    b = run_and_check(mods, clouds, poses, 0.05, linear=True)
    pa, pb = a["pushed"].view(np.uint32), b["pushed"].view(np.uint32)
    assert 0 < (pa != pb).any(axis=1).sum() < len(pa)   # the two orders round differently on some points: the flag is not a no-op


@pytest.mark.gpu
def test_gpu_a_keyframe_used_twice(mods, scene):
    rng = np.random.default_rng(15)
    clouds = [cloud(rng, 1500), cloud(rng, 700)]
    T0, T1, T2 = (pose(scene, rng, 50.0) for _ in range(3))
    g = fresh(mods, clouds)
    g.generate([T0, T1], [0, 1], 0.1)
    once, info = g.to_numpy(), g.info()
    g.generate([T0, T1, T0], [0, 1, 0], 0.1)   # the same pose again: nothing new, no other origin
    assert same_f32(g.to_numpy(), once) and same_f64(g.info()["min"], info["min"]) and g.info()["n_pushed"] == info["n_pushed"] + 1500
    assert_equals(g, mnp.generate([clouds[0], clouds[1], clouds[0]], [T0, T1, T0], 0.1))
    g.generate([T0, T2], [0, 0], 0.1)          # two poses: the union
    want = mnp.generate([clouds[0], clouds[0]], [T0, T2], 0.1)
    assert_equals(g, want)
    parts = [mnp.keys_of(mnp.push([clouds[0]], [T]), want["min"], 0.1) for T in (T0, T2)]
    union = np.unique(mnp.interleave(np.concatenate(parts), want["depth"]))
    assert np.array_equal(union, want["keys"]) and g.n == len(union)


@pytest.mark.gpu
def test_gpu_handle_reuse_and_clear(mods, scene):
    rng = np.random.default_rng(16)
    clouds = [cloud(rng, n, beyond=1) for n in (5000, 0, 1200, 300)]
    poses = [pose(scene, rng) for _ in clouds]
    other = [pose(scene, rng) for _ in clouds]
    g = fresh(mods, clouds)
    calls = [(poses, [0, 1, 2, 3], 0.05, False), ([other[2], other[0]], [2, 0], 0.0, False), ([other[3]], [3], 0.3, True), (other, [3, 2, 1, 0], 0.1, False)]
    sizes = []
    for ps, ids, res, linear in calls:   # a big octree, the raw cloud, a much smaller octree, another one: the same as a fresh handle every time
        g.generate(ps, ids, res, linear)
        got, info = g.to_numpy(), g.info()
        f = fresh(mods, clouds)
        f.generate(ps, ids, res, linear)
        assert same_f32(got, f.to_numpy()) and info["n_out"] == f.info()["n_out"] and same_f64(info["min"], f.info()["min"]) and info["depth"] == f.info()["depth"]
        assert_equals(g, mnp.generate([clouds[i] for i in ids], ps, res, linear), got)
        sizes.append(g.n)
    assert sizes[2] < sizes[1] < sizes[0]
    g.clear()
    assert g.points().n == 0 and g.info()["n_out"] == 0
    with pytest.raises(mods[0].ApdgicpError):
        g.generate([I4], [0], 0.05)          # an unknown id now
    assert g.add_keyframe(clouds[2]) == 0    # ids start again
    g.generate([other[1]], None, 0.05)
    assert_equals(g, mnp.generate([clouds[2]], [other[1]], 0.05))


@pytest.mark.gpu
def test_gpu_argument_errors(mods):
    reg = mods[0]
    g = fresh(mods, [np.zeros((3, 4), dtype=F32)])
    for args in (([], []), ([I4], [1]), ([I4], [-1])):
        with pytest.raises(reg.ApdgicpError) as e:
            g.generate(*args)
        assert e.value.code == -1
    with pytest.raises(reg.ApdgicpError):
        g.generate([I4], None, float("nan"))
    assert g.generate([I4], None, 0.05) == 1   # still usable


@pytest.mark.gpu
def test_gpu_inputs_strides_and_intensity(mods, scene):
    """16- and 32-byte rows, the intensity at byte 12, at byte 16 or absent, host arrays and device tensors: all the same cloud"""
    import torch
    rng = np.random.default_rng(17)
    c = cloud(rng, 2100, beyond=3)
    T = pose(scene, rng)
    wide = np.zeros((len(c), 8), dtype=F32)   # pcl::PointXYZI: {x, y, z, pad, intensity, pad[3]}
    wide[:, :3], wide[:, 3], wide[:, 4], wide[:, 5:] = c[:, :3], -1.0, c[:, 3], -2.0
    want = mnp.generate([c], [T], 0.0)
    bare = mnp.generate([c[:, :3]], [T], 0.0)
    assert (want["points"][:, 3] != 0).all() and (bare["points"][:, 3] == 0).all()
    for arr, col, exp in ((c, 3, want), (wide, 4, want), (c, None, bare), (np.ascontiguousarray(c[:, :3]), 3, bare), (wide, None, bare)):
        for dev in (False, True):
            g = mods[1].MapCloudGenerator()
            g.add_keyframe(torch.from_numpy(arr).cuda() if dev else arr, intensity_column=col)
            g.generate([T], None, 0.0)
            assert_equals(g, exp)
    t = torch.from_numpy(wide).cuda()
    g = mods[1].MapCloudGenerator()
    g.add_keyframe(t, intensity_column=4)
    t.zero_()   # the object owns a copy
    torch.cuda.synchronize()
    g.generate([T], None, 0.05)
    assert_equals(g, mnp.generate([c], [T], 0.05))


@pytest.mark.gpu
def test_gpu_depth_limit_is_reported_and_the_handle_survives(mods, scene):
    reg = mods[0]
    p = np.array([[1.0, 2.0, 0.5, 9.0]], dtype=F32)
    c1 = cloud(np.random.default_rng(18), 100)
    g = fresh(mods, [p, c1])
    far = scene.make_transform(np.array([3.0e5, 0.0, 0.0]))
    with pytest.raises(mnp.DepthLimit):
        mnp.generate([p, p], [I4, far], 0.05)
    with pytest.raises(reg.ApdgicpError) as e:
        g.generate([I4, far], [0, 0], 0.05)
    assert e.value.code == -5 and "21 levels" in str(e.value) and g.points().n == 0
    assert g.generate([I4, far], [0, 0], 0.5) == 2   # 6e5 voxels: depth 20
    assert_equals(g, mnp.generate([p, p], [I4, far], 0.5))
    g.generate([I4, I4], [0, 1], 0.05)
    assert_equals(g, mnp.generate([p, c1], [I4, I4], 0.05))


@pytest.fixture(scope="module")
def trajectory(scene):
    return mnp.trajectory_keyframes(scene, 32, 8192, 20250101, n_distinct=8, origin=(250.0, -120.0, 3.0))


@pytest.mark.gpu
@pytest.mark.parametrize("res", [0.05, 0.3])
def test_gpu_thirty_two_keyframes_on_a_trajectory(mods, trajectory, res):
    clouds, poses = trajectory
    g = fresh(mods, clouds)
    g.generate(poses, None, res)
    want = mnp.generate(clouds, poses, res)
    assert_equals(g, want)
    assert want["n_input"] == 32 * 8192 and 0 < want["n_pushed"] < want["n_input"] and want["rounds"] >= 1 and 1000 < want["n_out"] < want["n_pushed"]
    assert g.info()["sort_passes"] == (3 * want["depth"] + 7) // 8


@pytest.mark.gpu
def test_gpu_map_cloud_becomes_a_registration_target(mods, scene):
    """the device pointer of points() goes to FastAPDGICP.setInputTarget and a scan registers against it like against the same cloud
    handed over from the host (the oracle on the same points; the pose error bar is smoke()'s)"""
    import ref
    reg = mods[0]
    src, tgt, _, guess = scene.make_pair(2048, 4096, scene.pair_seed(0, 0), "odometry")
    g = fresh(mods, [tgt])
    assert g.generate([I4], None, 0.05) > 1000
    target = g.to_numpy()
    kw = dict(max_correspondence_distance=2.0, transformation_epsilon=0.01, azimuth_variance_deg=1.0)
    a = reg.FastAPDGICP(reg.default_params(**kw), device=0)
    a.setInputSource(src)
    a.setInputTarget(g.points())
    T = a.align(guess)
    o = ref.RefAPDGICP(ref.default_params(**kw))
    o.setInputSource(src)
    o.setInputTarget(np.ascontiguousarray(target[:, :3]))
    To = o.align(guess)
    te, re_ = scene.pose_error(To, T)
    assert a.hasConverged() and o.hasConverged() and te <= 1e-3 and re_ <= 1e-4
