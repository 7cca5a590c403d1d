"""Scan preprocessing on the device (riv-slam_amd/scan_filter.py, csrc/apd_filter.hpp): the range gate, the voxel grid and the
outlier filters of PreprocessingNodelet::cloud_callback (preprocessing_nodelet.cpp:812-815).

The expected values come from tests/scan_filter_np.py, a numpy restatement of include/apdgicp_hip.h's "scan preprocessing" section
(PCL as published; PCL is not installed here).  Its k-NN distances come from the checker's kd-tree (ref.RefAPDGICP.knn_kdtree_batch,
pinned bit for bit to the reference tree's nanoflann by tests/test_oracle.py) and, on the CPU, from a chunked numpy brute force in FLANN
L2_Simple order.

Bars (GPU): gate -- kept indices and output exact; voxel grid -- byte-equal to a one-cloud identity-pose apdgicp_submap_assemble and
the bars of tests/test_submap.py against the checker; STATISTICAL -- every score bit for bit, mean / stddev / thr within 1e-9 relative
of the sequential restatement (the device adds the n <= 2^17 doubles in a fixed tree, PCL one after the other), the kept mask
identical after asserting on the restatement alone that no score lies within 1e-9 thr of thr; RADIUS -- d2[k-1] bit for bit, no value
equal to r^2, the mask identical.  Those two conditions keep `<=` away from equality on the scene's scans; the line and the lattice of
"inputs that sit on the threshold" put every statistic exactly on it.
"""
import importlib
import os
import subprocess

import numpy as np
import pytest

import ref as R
from scan_filter_np import knn_d2_brute, knn_d2_kdtree, np_radius, np_range_gate, np_statistical

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
NEW_SYMBOLS = ["apdgicp_scan_filter_default_params", "apdgicp_scan_filter_create", "apdgicp_scan_filter_destroy", "apdgicp_scan_filter_set_params",
               "apdgicp_scan_filter_run", "apdgicp_scan_filter_points", "apdgicp_scan_filter_copy", "apdgicp_scan_filter_stage_counts",
               "apdgicp_scan_filter_scores"]

def bench_scene_with_clutter(scene, n, share=0.05, seed=0):
    """the bench scene (bench.py's pair generator) with `share` of the points replaced by clutter spread over the frustum"""
    src = scene.make_pair(n, 16, scene.pair_seed(0, seed), "odometry")[0]
    rng = np.random.default_rng(77 + seed)
    m = int(share * n)
    r, az, el = rng.uniform(2, 100, m), rng.uniform(-scene.AZ_MAX, scene.AZ_MAX, m), rng.uniform(-scene.EL_MAX, scene.EL_MAX, m)
    src = src.copy()
    src[rng.choice(n, m, replace=False)] = np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)], 1).astype(F32)
    return np.ascontiguousarray(np.concatenate([src, rng.uniform(0, 40, (n, 1)).astype(F32)], 1))


def with_duplicates(scene):
    c = scene.raw_scan(2048, 5)
    c[1000:1300] = c[:300]
    return c


def input_clouds(scene):
    return {"raw700": scene.raw_scan(700, 1), "raw2048": scene.raw_scan(2048, 2), "raw8192": scene.raw_scan(8192, 3), "raw16384": scene.raw_scan(16384, 4),
            "bench8192": bench_scene_with_clutter(scene, 8192), "bench2048": bench_scene_with_clutter(scene, 2048), "dup2048": with_duplicates(scene)}


CLOUD_NAMES = ("raw700", "raw2048", "raw8192", "raw16384", "bench8192", "bench2048", "dup2048")


# ------------------------------------------------------------------ CPU
def test_raw_scan_is_what_preprocessing_sees(scene):
    c = scene.raw_scan(8192, 3)
    assert c.shape == (8192, 4) and c.dtype == F32 and np.array_equal(c, scene.raw_scan(8192, 3), equal_nan=True)
    fin = np.isfinite(c[:, :3]).all(1)
    d = np.linalg.norm(c[fin, :3].astype(np.float64), axis=1)
    assert (~fin).sum() == 5 and (d < 2.0).sum() >= 200 and (d > 100.0).sum() >= 150
    keep = np_range_gate(c)
    assert 0.9 * 8192 < keep.sum() < 8192 - 300 and not keep[~fin].any()


@pytest.mark.parametrize("name", ("raw2048", "bench2048", "dup2048"))
def test_the_two_restatements_agree(scene, name):
    """kd-tree distances (the checker) against numpy brute force: scores, thresholds and masks exactly equal"""
    c = input_clouds(scene)[name]
    c = c[np_range_gate(c)]
    for k in (2, 6, 21, 32):
        a, b = knn_d2_kdtree(c, k), knn_d2_brute(c, k)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and not a[:, 0].any()
        for mul in (0.5, 1.0, 2.0):
            ra, rb = np_statistical(a, k - 1, mul), np_statistical(b, k - 1, mul)
            assert np.array_equal(ra[0].view(np.uint32), rb[0].view(np.uint32)) and ra[1:4] == rb[1:4] and np.array_equal(ra[4], rb[4])
            assert 0 < ra[4].sum() < len(c)
    for radius, mn in ((0.8, 2), (0.5, 5)):
        sa, ma = np_radius(knn_d2_kdtree(c, mn + 1), mn, radius)
        sb, mb = np_radius(knn_d2_brute(c, mn + 1), mn, radius)
        assert np.array_equal(sa.view(np.uint32), sb.view(np.uint32)) and np.array_equal(ma, mb) and 0 < ma.sum() < len(c)


# ---- the outlier filters at a controlled n2: no gate, no voxel grid and a finite input, so the filter sees the n rows it is given
EDGE_SEED = 6     # chosen on the CPU: no case below has a score within 1e-9 thr of thr or a statistic equal to r^2 (asserted)
# around: 4 queries per wave of k_knn_stat_coop, 64-lane waves, the 1024-thread compaction blocks, the cloud sort's classes (2048, 16384)
EDGE_SIZES = ("k", "k+1", 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 16383, 16384, 16385)
EDGE_MEAN_K = (1, 20, 31)
EDGE_RADIUS = ((0.8, 2), (2.0, 20))
_edge_cache = {}


def edge_size(size, k):
    return {"k": k, "k+1": k + 1}.get(size, size)


def edge_scan(scene, n):
    if "scan" not in _edge_cache:
        c = scene.raw_scan(20000, EDGE_SEED)
        _edge_cache["scan"] = np.ascontiguousarray(c[np.isfinite(c).all(1)])
    return _edge_cache["scan"][:n]


def edge_d2(scene, n, k):
    """the restatement's k-NN distances of the first n finite rows: computed once, shared by the CPU and the GPU tests"""
    if (n, k) not in _edge_cache:
        d2 = knn_d2_kdtree(edge_scan(scene, n), k)
        d2.setflags(write=False)
        _edge_cache[n, k] = d2
    return _edge_cache[n, k]


def statistical_expected(d2, mean_k, mul):
    score, mean, stddev, thr, keep = np_statistical(d2, mean_k, mul)
    gap = np.abs(score.astype(np.float64) - thr).min()
    assert gap > 1e-9 * thr, "the input has a score on the threshold: choose another cloud"   # a condition on the input
    return score, mean, stddev, thr, keep, gap


def radius_expected(d2, mn, radius):
    stat, keep = np_radius(d2, mn, radius)
    assert not (stat.astype(np.float64) == radius * radius).any()   # a condition on the input
    return stat, keep


def line_cloud(n):
    c = np.zeros((n, 4), dtype=F32)
    c[:, 0] = F32(0.5) * np.arange(n, dtype=F32)
    c[:, 3] = np.arange(n, dtype=F32)
    return c


def lattice_cloud():
    """8 x 8 x 8 points 0.5 apart from -2.0 (they straddle the origin), shuffled; every coordinate and every distance is exact in fp32"""
    g = (F32(-2.0) + F32(0.5) * np.arange(8, dtype=F32)).astype(F32)
    xyz = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    c = np.concatenate([xyz, np.arange(512, dtype=F32)[:, None]], 1)
    return np.ascontiguousarray(c[np.random.default_rng(8).permutation(512)], dtype=F32)


LINE_SIZES = (2, 3, 64, 65, 1025)
LATTICE_RADIUS_KEPT = {3: 512, 4: 504, 5: 432, 6: 216}   # corners, then edges, then faces go
LATTICE_MEAN_K6_KEPT = {0.5: 432, 1.0: 432, 2.0: 504}


def test_controlled_sizes_meet_the_input_conditions(scene):
    assert len(edge_scan(scene, 20000)) >= 16385
    for size in EDGE_SIZES:
        for mean_k in EDGE_MEAN_K:
            n = edge_size(size, mean_k + 1)
            statistical_expected(edge_d2(scene, n, mean_k + 1), mean_k, 1.0)
        for radius, mn in EDGE_RADIUS:
            n = edge_size(size, mn + 1)
            radius_expected(edge_d2(scene, n, mn + 1), mn, radius)
    few = scene.raw_scan(2048, 9)
    few = np.ascontiguousarray(few[np.isfinite(few).all(1)][:15])
    statistical_expected(knn_d2_kdtree(few, 15), 14, 1.0)   # test_edge_cases' n2 = k = 15


@pytest.mark.parametrize("knn", (knn_d2_kdtree, knn_d2_brute))
def test_threshold_inputs_sit_on_the_threshold(knn):
    """the numbers the GPU tests assert as literals, from the restatement: every statistic EQUAL to the threshold, so `<=` keeps all"""
    for n in LINE_SIZES:
        for mul in (0.5, 1.0, 2.0):
            score, mean, stddev, thr, keep = np_statistical(knn(line_cloud(n), 2), 1, mul)
            assert (score == F32(0.5)).all() and (mean, stddev, thr) == (0.5, 0.0, 0.5) and keep.all()
    c = lattice_cloud()
    assert c[:, :3].min() == -2.0 and c[:, :3].max() == 1.5 and len(np.unique(c[:, :3], axis=0)) == 512
    for mn, kept in LATTICE_RADIUS_KEPT.items():
        stat, keep = np_radius(knn(c, mn + 1), mn, 0.5)
        assert keep.sum() == kept and np.array_equal(keep, stat == F32(0.25)) and set(np.unique(stat)) <= {F32(0.25), F32(0.5)}
    score, mean, stddev, thr, keep = np_statistical(knn(c, 4), 3, 1.0)
    assert (score == F32(0.5)).all() and (mean, stddev, thr) == (0.5, 0.0, 0.5) and keep.all()
    for mul, kept in LATTICE_MEAN_K6_KEPT.items():
        score, mean, stddev, thr, keep, gap = statistical_expected(knn(c, 7), 6, mul)
        assert len(np.unique(score)) == 4 and keep.sum() == kept


@pytest.fixture(scope="module")
def mods():
    import __graft_entry__ as g
    g.build()
    return (importlib.import_module("riv-slam_amd.registration"), importlib.import_module("riv-slam_amd.scan_filter"),
            importlib.import_module("riv-slam_amd.submap"))


def test_symbols_are_exported_and_defaults_are_the_nodelets(mods):
    reg, sf, _ = mods
    L = reg.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name) and name in reg.SYMBOLS
    p = sf.default_filter_params()   # preprocessing_nodelet.cpp:137-205
    assert (p.use_distance_filter, p.near, p.far, p.z_low, p.z_high) == (1, 1.0, 100.0, -5.0, 20.0)
    assert list(p.leaf) == [F32(0.1)] * 3 and (p.outlier_method, p.mean_k, p.stddev_mul) == (sf.OUTLIER_STATISTICAL, 20, 1.0)
    assert (p.radius, p.min_neighbors) == (0.8, 2)
    import ctypes
    assert ctypes.sizeof(sf.ScanFilterParams) == 4 * 4 + 6 * 8 + 3 * 4 + 4
    q = sf.default_filter_params(leaf=None, outlier_method="radius")
    assert list(q.leaf) == [0.0] * 3 and q.outlier_method == sf.OUTLIER_RADIUS


def test_no_gpu_fails_loudly(mods, scene):
    """without a device the class raises (there is no CPU fall-back); with one it is created and runs"""
    import torch
    reg, sf, _ = mods
    if torch.cuda.is_available():
        assert 0 < sf.ScanFilter().run(scene.raw_scan(700, 1)) < 700
    else:
        with pytest.raises(reg.ApdgicpError):
            sf.ScanFilter()


def build_cpp():
    import __graft_entry__ as g
    g.build()
    exe = os.path.join(ROOT, "tests", "cpp", "_build", "test_scan_filter")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    lib_dir = os.path.join(ROOT, "riv-slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "tests", "pcl_shim"), "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "riv-slam_amd", "cpp"), os.path.join(ROOT, "tests", "cpp", "test_scan_filter.cpp"),
                           "-L", lib_dir, "-lapdgicp_hip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-o", exe])
    return exe


def test_cpp_class_compiles_against_the_pcl_shim():
    out = subprocess.run([build_cpp()], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "compile-only" in out.stdout


# ------------------------------------------------------------------ GPU
def centroids_close(a, b, cnt=None):
    """tests/test_submap.py's bar: fp32 sums of `cnt` values added in another order"""
    k = 4.0 if cnt is None else np.maximum(cnt, 4)[:, None].astype(np.float64)
    return bool((np.abs(a.astype(np.float64) - b) <= k * np.finfo(F32).eps * np.maximum(np.abs(b), 1.0)).all())


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CLOUD_NAMES)
def test_range_gate(mods, scene, name):
    reg, sf, _ = mods
    c = input_clouds(scene)[name]
    f = sf.ScanFilter(leaf=None, outlier_method="NONE")
    for near, far, zl, zh in ((1.0, 100.0, -5.0, 20.0), (2.0, 50.0, -1.0, 3.0), (0.0, 1e9, -1e9, 1e9), (30.0, 31.0, -5.0, 20.0), (5.0, 4.0, 0.0, 1.0)):
        f.set_params(near=near, far=far, z_low=zl, z_high=zh)
        keep = np_range_gate(c, near, far, zl, zh)
        n = f.run(c)
        print(f"{name} gate {near} {far} {zl} {zh}: kept {n} of {len(c)}")
        assert n == keep.sum() and np.array_equal(bits(f.to_numpy()), bits(c[keep]))
        assert f.stage_counts() == (len(c), n, n, n)
    # no gate, no leaf: removeNaNFromPointCloud, order kept
    f.set_params(use_distance_filter=0)
    fin = np.isfinite(c[:, :3]).all(1)
    assert f.run(c) == fin.sum() and np.array_equal(bits(f.to_numpy()), bits(c[fin])) and f.stage_counts()[1] == len(c)
    # a threshold that sits exactly on a point's fp32 norm: strict comparisons drop it on either side
    x, y, z = c[fin][0, :3]
    d = float(np.sqrt((x * x + y * y) + z * z))
    f.set_params(use_distance_filter=1, near=d, far=1e9, z_low=-1e9, z_high=1e9)
    assert f.run(c) == np_range_gate(c, d, 1e9, -1e9, 1e9).sum()
    f.set_params(near=0.0, far=d)
    assert f.run(c) == np_range_gate(c, 0.0, d, -1e9, 1e9).sum()


@pytest.mark.gpu
@pytest.mark.parametrize("name", CLOUD_NAMES)
def test_downsample_is_the_submap_voxel_grid(mods, scene, name):
    reg, sf, sub = mods
    c = input_clouds(scene)[name]
    a = sub.SubmapAssembler()
    f = sf.ScanFilter(outlier_method="NONE", use_distance_filter=0)
    for leaf in (0.1, 0.25, (0.2, 0.4, 1.0), 5.0):
        f.set_params(leaf=leaf, use_distance_filter=0)
        n = f.run(c)
        got = f.to_numpy()
        exp, idx, cnt = R.submap_assemble([c], None, leaf)
        if (idx == -1).all():
            # the ungated scan reaches 180 m: "Leaf size is too small for the input dataset", PCL returns its input -- the filter
            # returns it without its non-finite points, in input order (include/apdgicp_hip.h)
            fin = np.isfinite(c[:, :3]).all(1)
            assert a.assemble([c], None, leaf) == len(c) and n == fin.sum() and np.array_equal(bits(got), bits(c[fin]))
        else:
            assert n == a.assemble([c], None, leaf) and np.array_equal(bits(got), bits(a.to_numpy()))   # the same kernels
            assert n == exp.shape[0]
            single = cnt == 1
            assert np.array_equal(got[single], exp[single]) and centroids_close(got, exp, cnt)
        # behind the gate: the voxel grid of the gated cloud
        f.set_params(use_distance_filter=1)
        keep = np_range_gate(c)
        n = f.run(c)
        assert n == a.assemble([c[keep]], None, leaf) and np.array_equal(bits(f.to_numpy()), bits(a.to_numpy()))
        exp, idx, cnt = R.submap_assemble([c[keep]], None, leaf)
        assert n == exp.shape[0] and (idx >= 0).all() and np.array_equal(f.to_numpy()[cnt == 1], exp[cnt == 1]) and centroids_close(f.to_numpy(), exp, cnt)
        assert f.stage_counts() == (len(c), keep.sum(), n, n)
        print(f"{name} leaf {leaf}: {len(c)} -> {keep.sum()} -> {n}")


def step2_cloud(sf, c, leaf):
    f = sf.ScanFilter(outlier_method="NONE", leaf=leaf)
    f.run(c)
    return f.to_numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", CLOUD_NAMES)
def test_statistical_outlier_removal(mods, scene, name):
    """The bar on mean / stddev / thr is 1e-9 relative: the device adds the scores in a fixed tree, the restatement (like PCL) one after
    the other, and the rounding of a sum of n <= 2^17 doubles is ~n 1.1e-16 = 1.5e-11 at worst.  Largest difference observed on an
    MI355X over all 84 cases of this test: 0 -- the scores are fp32 values within a few binades of each other, so sums of up to 15 340
    of them (and of their fp32 squares) are exact in fp64 in either order.  Each case prints its own figure."""
    reg, sf, _ = mods
    c = input_clouds(scene)[name]
    leaf = None if name == "dup2048" else 0.1   # (the voxel grid would merge the duplicates)
    s2 = step2_cloud(sf, c, leaf)
    f = sf.ScanFilter(leaf=leaf)
    worst = 0.0
    for mean_k in (1, 5, 20, 31):
        d2 = knn_d2_kdtree(s2, mean_k + 1)
        for mul in (0.5, 1.0, 2.0):
            score, mean, stddev, thr, keep = np_statistical(d2, mean_k, mul)
            gap = np.abs(score.astype(np.float64) - thr).min()
            assert gap > 1e-9 * thr, "the input has a score on the threshold: choose another cloud"   # a condition on the input
            f.set_params(mean_k=mean_k, stddev_mul=mul)
            n = f.run(c)
            sc = f.scores()
            rel = max(abs(sc["mean"] - mean) / mean, abs(sc["stddev"] - stddev) / stddev, abs(sc["thr"] - thr) / thr)
            worst = max(worst, rel)
            print(f"{name} mean_k {mean_k} mul {mul}: n2 {len(s2)} kept {keep.sum()} ({keep.mean():.3f}) thr {thr:.6f} nearest score {gap / thr:.2e} thr away, "
                  f"sums rel diff {rel:.2e}, score bits equal {np.array_equal(bits(sc['stat']), bits(score))}")
            assert np.array_equal(bits(sc["stat"]), bits(score))
            assert rel <= 1e-9
            assert np.array_equal(sc["kept"], keep) and n == keep.sum()
            assert np.array_equal(bits(f.to_numpy()), bits(s2[keep]))
            assert f.stage_counts()[2:] == (len(s2), n)
    print(f"{name}: largest relative difference of mean / stddev / thr {worst:.3e}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", CLOUD_NAMES)
def test_radius_outlier_removal(mods, scene, name):
    reg, sf, _ = mods
    c = input_clouds(scene)[name]
    leaf = None if name == "dup2048" else 0.1
    s2 = step2_cloud(sf, c, leaf)
    f = sf.ScanFilter(leaf=leaf, outlier_method="RADIUS")
    for radius, mn in ((0.8, 2), (0.5, 5)):
        stat, keep = np_radius(knn_d2_kdtree(s2, mn + 1), mn, radius)
        assert not (stat.astype(np.float64) == radius * radius).any()   # a condition on the input
        f.set_params(radius=radius, min_neighbors=mn)
        n = f.run(c)
        sc = f.scores()
        print(f"{name} radius {radius} min_neighbors {mn}: n2 {len(s2)} kept {keep.sum()} ({keep.mean():.3f}), nearest to r^2 {np.abs(stat.astype(np.float64) - radius * radius).min():.2e}")
        assert np.array_equal(bits(sc["stat"]), bits(stat)) and sc["thr"] == radius * radius
        assert np.array_equal(sc["kept"], keep) and n == keep.sum() and np.array_equal(bits(f.to_numpy()), bits(s2[keep]))


def assert_statistical(f, c, s2, d2, mean_k, mul, tag):
    """test_statistical_outlier_removal's bars for one run of `f` on `c`; s2: the cloud the outlier filter sees, d2: its k-NN distances"""
    score, mean, stddev, thr, keep, gap = statistical_expected(d2, mean_k, mul)
    f.set_params(outlier_method="STATISTICAL", mean_k=mean_k, stddev_mul=mul)
    n = f.run(c)
    sc = f.scores()
    rel = max(abs(sc["mean"] - mean) / mean, abs(sc["stddev"] - stddev) / stddev, abs(sc["thr"] - thr) / thr)
    print(f"{tag} mean_k {mean_k} mul {mul}: n2 {len(s2)} kept {keep.sum()} thr {thr:.6f} nearest score {gap / thr:.2e} thr away, sums rel diff {rel:.2e}, "
          f"score bits equal {np.array_equal(bits(sc['stat']), bits(score))}")
    assert np.array_equal(bits(sc["stat"]), bits(score))
    assert rel <= 1e-9
    assert np.array_equal(sc["kept"], keep) and n == keep.sum()
    assert np.array_equal(bits(f.to_numpy()), bits(s2[keep]))
    assert f.stage_counts()[2:] == (len(s2), n)
    return rel


def assert_radius(f, c, s2, d2, mn, radius, tag):
    """test_radius_outlier_removal's bars for one run of `f` on `c`"""
    stat, keep = radius_expected(d2, mn, radius)
    f.set_params(outlier_method="RADIUS", radius=radius, min_neighbors=mn)
    n = f.run(c)
    sc = f.scores()
    print(f"{tag} radius {radius} min_neighbors {mn}: n2 {len(s2)} kept {keep.sum()}, stat bits equal {np.array_equal(bits(sc['stat']), bits(stat))}")
    assert np.array_equal(bits(sc["stat"]), bits(stat)) and sc["thr"] == radius * radius
    assert np.array_equal(sc["kept"], keep) and n == keep.sum() and np.array_equal(bits(f.to_numpy()), bits(s2[keep]))
    assert f.stage_counts()[2:] == (len(s2), n)


@pytest.mark.gpu
@pytest.mark.parametrize("size", EDGE_SIZES, ids=str)
def test_statistical_at_controlled_sizes(mods, scene, size):
    """n2 = the input size (leaf None, no gate, finite rows); the bars and their derivation are test_statistical_outlier_removal's"""
    reg, sf, _ = mods
    f = sf.ScanFilter(leaf=None, use_distance_filter=0)
    for mean_k in EDGE_MEAN_K:
        n = edge_size(size, mean_k + 1)
        if n < mean_k + 1:
            continue
        c = edge_scan(scene, n)
        assert_statistical(f, c, c, edge_d2(scene, n, mean_k + 1), mean_k, 1.0, f"n2 {n}")


@pytest.mark.gpu
@pytest.mark.parametrize("size", EDGE_SIZES, ids=str)
def test_radius_at_controlled_sizes(mods, scene, size):
    reg, sf, _ = mods
    f = sf.ScanFilter(leaf=None, use_distance_filter=0, outlier_method="RADIUS")
    for radius, mn in EDGE_RADIUS:
        n = edge_size(size, mn + 1)
        if n < mn + 1:
            continue
        c = edge_scan(scene, n)
        assert_radius(f, c, c, edge_d2(scene, n, mn + 1), mn, radius, f"n2 {n}")


def knn_mode(monkeypatch, mode):
    if mode == "brute":
        monkeypatch.setenv("APDGICP_KNN_MODE", "brute")   # (read when the filter's engine is created: a new ScanFilter per mode)
    else:
        monkeypatch.delenv("APDGICP_KNN_MODE", raising=False)


def assert_all_on_the_threshold(f, c, thr):
    """every statistic EQUALS the threshold, so `<=` keeps every point and `<` none; == throughout: the sums are exact in any order"""
    n = f.run(c)
    sc = f.scores()
    assert (sc["stat"] == F32(thr)).all() and sc["thr"] == thr
    assert sc["kept"].all() and n == len(c) and np.array_equal(bits(f.to_numpy()), bits(c))
    assert f.stage_counts() == (len(c), len(c), len(c), len(c))
    return sc


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ("pruned", "brute"))
def test_statistical_keeps_scores_equal_to_the_threshold(mods, monkeypatch, mode):
    """Points 0.5 apart on a line, mean_k = 1: every score is exactly 0.5, their sum 0.5 n and the sum of squares 0.25 n in any order, so
    mean = 0.5, stddev = 0 and thr = 0.5 = every score, whatever stddev_mul.  The lattice with mean_k = 3 is the same in three dimensions."""
    reg, sf, _ = mods
    knn_mode(monkeypatch, mode)
    f = sf.ScanFilter(leaf=None, use_distance_filter=0, mean_k=1)
    for n in LINE_SIZES:
        for mul in (0.5, 1.0, 2.0):
            f.set_params(stddev_mul=mul)
            sc = assert_all_on_the_threshold(f, line_cloud(n), 0.5)
            assert (sc["mean"], sc["stddev"], sc["thr"]) == (0.5, 0.0, 0.5)
    c = lattice_cloud()
    f.set_params(mean_k=3, stddev_mul=1.0)
    sc = assert_all_on_the_threshold(f, c, 0.5)
    assert (sc["mean"], sc["stddev"], sc["thr"]) == (0.5, 0.0, 0.5)
    d2 = knn_d2_kdtree(c, 7)
    for mul, kept in LATTICE_MEAN_K6_KEPT.items():   # four distinct scores (corner, edge, face, inside), none on the threshold
        assert_statistical(f, c, c, d2, 6, mul, f"lattice {mode}")
        assert f.n == kept


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ("pruned", "brute"))
def test_radius_keeps_distances_equal_to_the_radius(mods, monkeypatch, mode):
    """The lattice with radius = 0.5 = its spacing: d2 to a face neighbour is 0.25 = r^2 exactly, to the next one 0.5.  A corner has 3
    face neighbours, an edge point 4, a face point 5, an inner point 6."""
    reg, sf, _ = mods
    knn_mode(monkeypatch, mode)
    c = lattice_cloud()
    f = sf.ScanFilter(leaf=None, use_distance_filter=0, outlier_method="RADIUS", radius=0.5, min_neighbors=3)
    assert_all_on_the_threshold(f, c, 0.25)
    for mn, kept in LATTICE_RADIUS_KEPT.items():
        stat, keep = np_radius(knn_d2_kdtree(c, mn + 1), mn, 0.5)
        f.set_params(min_neighbors=mn)
        n = f.run(c)
        sc = f.scores()
        assert np.array_equal(bits(sc["stat"]), bits(stat)) and sc["thr"] == 0.25
        assert n == kept == keep.sum() and np.array_equal(sc["kept"], keep) and np.array_equal(bits(f.to_numpy()), bits(c[keep]))
        assert np.array_equal(sc["kept"], sc["stat"] == F32(0.25))   # kept: exactly the points whose statistic equals r^2


def cloud_past_1024_blocks():
    """1024 * 1024 + 1025 rows, ranges 0 .. 200 m so that the default gate keeps about half, 300 rows with a NaN or an infinity on both
    sides of row 1 048 576 (the first row of compaction block 1024)"""
    n, edge = 1024 * 1024 + 1025, 1024 * 1024
    rng = np.random.default_rng(1_048_577)
    r, az = rng.uniform(0.0, 200.0, n), rng.uniform(-np.pi, np.pi, n)
    c = np.stack([r * np.cos(az), r * np.sin(az), rng.uniform(-4.0, 15.0, n), rng.uniform(0.0, 40.0, n)], 1).astype(F32)
    bad = np.concatenate([edge - 1 - rng.choice(5000, 150, replace=False), edge + rng.choice(1025, 150, replace=False)])
    c[bad, rng.integers(0, 3, 300)] = rng.choice(np.array([np.nan, np.inf, -np.inf], dtype=F32), 300)
    return np.ascontiguousarray(c), edge


@pytest.mark.gpu
def test_compaction_past_1024_blocks(mods):
    """scan_filter_compact's per-block counts are scanned by k_scan_bsum in passes of 1024 blocks with a running total carried from one
    pass into the next: 1026 blocks of 1024 rows take the second pass.  Points are kept on both sides of row 1 048 576 and the first 1024
    blocks keep some rows but not all, so a wrong carry moves the rows of blocks 1024 and 1025 (and the total).  No k-NN at this size."""
    reg, sf, _ = mods
    c, edge = cloud_past_1024_blocks()
    fin = np.isfinite(c[:, :3]).all(1)
    f = sf.ScanFilter(leaf=None, outlier_method="NONE")
    for gate in (1, 0):
        keep = np_range_gate(c) if gate else fin
        assert 0 < keep[:edge].sum() < edge and 0 < keep[edge:].sum() < len(c) - edge   # conditions on the input
        f.set_params(use_distance_filter=gate)
        n = f.run(c)
        print(f"gate {gate}: kept {n} of {len(c)}, {keep[:edge].sum()} in the first 1024 blocks, {keep[edge:].sum()} behind")
        assert n == keep.sum() and np.array_equal(bits(f.to_numpy()), bits(c[keep]))
        assert f.stage_counts() == (len(c), n if gate else len(c), n, n)
    assert 0.4 * len(c) < np_range_gate(c).sum() < 0.6 * len(c) and (~fin[:edge]).sum() == (~fin[edge:]).sum() == 150


@pytest.mark.gpu
def test_edge_cases(mods, scene):
    import torch
    reg, sf, _ = mods
    c = scene.raw_scan(2048, 9)
    # fewer points behind downsample than k
    f = sf.ScanFilter(leaf=None, use_distance_filter=0)
    few = np.ascontiguousarray(c[np.isfinite(c).all(1)][:15])
    with pytest.raises(reg.ApdgicpError) as e:
        f.run(few)
    assert e.value.code == -4   # APDGICP_ERR_TOO_FEW_POINTS
    assert_statistical(f, few, few, knn_d2_kdtree(few, 15), 14, 1.0, "few")   # n2 = k = 15: every point is a neighbour of every other
    with pytest.raises(reg.ApdgicpError) as e:
        f.set_params(mean_k=32)
    assert e.value.code == -5   # APDGICP_ERR_UNSUPPORTED
    # an all-NaN cloud, and an empty one: n_out = 0, status 0
    for f in (sf.ScanFilter(), sf.ScanFilter(leaf=None), sf.ScanFilter(use_distance_filter=0), sf.ScanFilter(leaf=None, use_distance_filter=0)):
        assert f.run(np.full((300, 4), np.nan, dtype=F32)) == 0 and f.to_numpy().shape == (0, 4) and f.points().n == 0
        assert f.stage_counts() == (300, 0 if f.params.use_distance_filter else 300, 0, 0)
        assert f.run(c[:0]) == 0
        assert f.run(c) > 0   # (and the object works on)
    # device-resident pcl::PointXYZI layout: 32-byte points, intensity at byte 16; xyz only: intensity 0
    f = sf.ScanFilter()
    n = f.run(c)
    want = f.to_numpy()
    t = torch.zeros((len(c), 8), dtype=torch.float32)
    t[:, :3] = torch.from_numpy(c[:, :3])
    t[:, 4] = torch.from_numpy(c[:, 3])
    assert f.run(t.cuda(), intensity_column=4) == n and np.array_equal(bits(f.to_numpy()), bits(want))
    assert f.run(torch.from_numpy(c).cuda()) == n and np.array_equal(bits(f.to_numpy()), bits(want))
    assert f.run(np.ascontiguousarray(c[:, :3]), intensity_column=None) == n
    got = f.to_numpy()
    assert np.array_equal(bits(got[:, :3]), bits(want[:, :3])) and not got[:, 3].any()
    # two runs, and a second object: byte-equal (scores, threshold and output)
    f.run(c)
    s1, o1 = f.scores(), f.to_numpy()
    g = sf.ScanFilter()
    g.run(c)
    f.run(c)
    for s in (f.scores(), g.scores()):
        assert np.array_equal(bits(s["stat"]), bits(s1["stat"])) and np.array_equal(s["kept"], s1["kept"]) and (s["mean"], s["stddev"], s["thr"]) == (s1["mean"], s1["stddev"], s1["thr"])
    assert np.array_equal(bits(f.to_numpy()), bits(o1)) and np.array_equal(bits(g.to_numpy()), bits(o1))


@pytest.mark.gpu
@pytest.mark.parametrize("method", ("STATISTICAL", "RADIUS"))
def test_brute_force_knn_gives_the_same_statistic(mods, scene, monkeypatch, method):
    """k = 21 (STATISTICAL 20 / RADIUS with 20 neighbours) through the pruned kernel and under APDGICP_KNN_MODE=brute"""
    reg, sf, _ = mods
    c = scene.raw_scan(8192, 3)
    kw = dict(outlier_method=method, mean_k=20, min_neighbors=20, radius=2.0)
    f = sf.ScanFilter(**kw)
    n = f.run(c)
    s = f.scores()
    monkeypatch.setenv("APDGICP_KNN_MODE", "brute")
    g = sf.ScanFilter(**kw)
    assert g.run(c) == n
    t = g.scores()
    assert np.array_equal(bits(s["stat"]), bits(t["stat"])) and np.array_equal(s["kept"], t["kept"]) and s["thr"] == t["thr"]
    assert np.array_equal(bits(f.to_numpy()), bits(g.to_numpy())) and 0 < n < f.stage_counts()[2]


@pytest.mark.gpu
def test_preprocess_and_set_source_feeds_the_registration(mods, scene):
    """cloud_callback's filters + setInputSource on the device against the same registration with the filtered cloud's host copy"""
    reg, sf, _ = mods
    import ctypes
    src, tgt, _, guess = scene.make_pair(8192, 8192, scene.pair_seed(0, 1), "odometry")
    raw = bench_scene_with_clutter(scene, 8192, seed=1)
    prm = reg.default_params(max_correspondence_distance=2.0, transformation_epsilon=0.01, azimuth_variance_deg=1.0)
    f = sf.ScanFilter()
    g = reg.FastAPDGICP(prm)
    g.setInputTarget(tgt)
    n = sf.preprocess_and_set_source(g, raw, f)
    assert 0 < n < 8192 and g.n_src == n
    T1 = g.align(guess)
    r1 = bytes(ctypes.string_at(ctypes.addressof(g.result), ctypes.sizeof(g.result)))
    h = reg.FastAPDGICP(prm)
    h.setInputTarget(tgt)
    h.setInputSource(f.to_numpy())
    T2 = h.align(guess)
    r2 = bytes(ctypes.string_at(ctypes.addressof(h.result), ctypes.sizeof(h.result)))
    assert g.hasConverged() and np.array_equal(T1, T2) and r1 == r2


@pytest.mark.gpu
def test_cpp_class_matches_python(mods, scene, tmp_path):
    reg, sf, _ = mods
    exe = build_cpp()
    c = scene.raw_scan(8192, 3)
    path = tmp_path / "scan.bin"
    with open(path, "wb") as fh:
        np.array([len(c)], dtype=np.int32).tofile(fh)
        c.tofile(fh)
    for args, kw in ((["STATISTICAL"], dict()), (["RADIUS"], dict(outlier_method="RADIUS")), (["NONE"], dict(outlier_method="NONE"))):
        outp = tmp_path / "out.bin"
        out = subprocess.run([exe, str(path), str(outp)] + args, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr
        counts = tuple(int(v) for v in out.stdout.split()[:4])
        f = sf.ScanFilter(**kw)
        n = f.run(c)
        assert counts == f.stage_counts() and int(out.stdout.split()[4]) == 1   # (the device pointer holds the same cloud)
        got = np.fromfile(outp, dtype=F32).reshape(-1, 4)
        assert got.shape[0] == n and np.array_equal(bits(got), bits(f.to_numpy()))
