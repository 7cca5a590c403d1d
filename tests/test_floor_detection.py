"""Floor plane detection and under-floor removal on the device (riv-slam_amd/floor_detection.py, csrc/apd_floor.hpp):
radar_graph_slam::FloorDetectionNodelet (radar_graph_slam/apps/floor_detection_nodelet.cpp).

The expected values come from tests/floor_detection_np.py, a numpy restatement in the operation orders include/apdgicp_hip.h states, fed
the same table of random words.

Bars (GPU): clip mask, clipped cloud, sampled indices, bad flags, every hypothesis's four fp32 coefficients, every n_in[k], iterations,
skipped, winner, exhausted flag, accepted / rejected, published and raw coefficients, inlier index list and cloud, under-floor cloud:
identical / bit for bit.  The normal statistic |u_z| / |u|: within 1e-6 (the device's fp64 Jacobi sweeps and numpy's eigh differ in the
last bits); the keep mask is compared on every point whose restated statistic is further than 1e-6 from cos(normal_filter_thresh), the
points inside that band enter the later stages as the device decided them (the restatement takes the mask as input).  Asserted on the
restatement alone, before the GPU is touched: at most 0.5 % of the clipped points lie in that band, and no |n.p + d| of any hypothesis
lies within 1 ulp of the distance threshold.
"""
import functools
import importlib
import math
import os
import subprocess

import numpy as np
import pytest

import floor_detection_np as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
NEW_SYMBOLS = ["apdgicp_floor_default_params", "apdgicp_floor_create", "apdgicp_floor_destroy", "apdgicp_floor_set_params", "apdgicp_floor_reset", "apdgicp_floor_run",
               "apdgicp_floor_inliers", "apdgicp_floor_under_floor_filtered", "apdgicp_floor_copy", "apdgicp_floor_hypotheses", "apdgicp_floor_debug"]
BAND = 1e-6


@pytest.fixture(scope="module")
def mods():
    import __graft_entry__ as g
    g.build()
    return (importlib.import_module("riv-slam_amd.registration"), importlib.import_module("riv-slam_amd.floor_detection"),
            importlib.import_module("riv-slam_amd.scan_filter"))


def scene_mod():
    return importlib.import_module("riv-slam_amd.scene")


def words_for(K, seed=0):
    return np.random.default_rng(seed).integers(0, 2**32, (K, 3), dtype=np.uint32)


def filtered_count(scan, cfg):
    """(m, points in the band) of the restatement"""
    mask, tilted = F.clip(scan, cfg)
    if not cfg.use_normal_filtering:
        return int(mask.sum()), 0
    c = tilted[mask]
    if len(c) < cfg.normal_k:
        return 0, 0
    stat = F.normal_stat(c[:, :3], cfg.normal_k).astype(np.float64)
    thr = math.cos(cfg.normal_filter_thresh * math.pi / 180.0)
    return int((stat > thr).sum()), int((np.abs(stat - thr) <= BAND).sum())


@functools.lru_cache(maxsize=None)
def scan_with_m(m, normal_filtering, tilt_deg, seed=21):
    """the shortest prefix of a floor_scan whose restated filtered count is exactly m (like scan_with_m of tests/test_ego_velocity.py).
    Without the normal filter the count is the height clip's and grows with the prefix; with it the count moves by about one per
    added point, so the prefix is found by stepping towards m -- and must have no point in the band, so that the device's m is m too."""
    cfg = F.Config(tilt_deg=tilt_deg, use_normal_filtering=normal_filtering)
    if normal_filtering and 0 < m < 50:
        # a sparse floor_scan passes the filter whole (ten neighbours metres apart always lie flat), so small counts are built: m floor
        # points in a 1 m patch, and 20 m away twelve points of a vertical wall patch, whose normals are horizontal
        rng = np.random.default_rng([seed, m])
        patch = np.stack([5.0 + rng.uniform(0, 1, m), rng.uniform(0, 1, m), -2.0 + 0.01 * rng.normal(size=m)], axis=1)
        wall = np.stack([25.0 + 0.01 * rng.normal(size=12), rng.uniform(0, 0.5, 12), rng.uniform(-2.9, -1.1, 12)], axis=1)
        a = np.deg2rad(tilt_deg)
        R = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
        xyz = np.concatenate([patch, wall], axis=0)[rng.permutation(m + 12)] @ R
        scan = np.ascontiguousarray(np.concatenate([xyz, rng.uniform(0, 40, (m + 12, 1))], axis=1).astype(F32))
        assert filtered_count(scan, cfg) == (m, 0)
        return scan
    big = scene_mod().floor_scan(max(512, 8 * m + 512), seed, tilt_deg=tilt_deg)
    mask, _ = F.clip(big, cfg)
    c = np.cumsum(mask)
    if not normal_filtering:
        if m == 0:
            return np.ascontiguousarray(big[~mask][:40])
        return np.ascontiguousarray(big[:int(np.searchsorted(c, m + 1))])
    if m == 0:
        return np.ascontiguousarray(big[:int(np.searchsorted(c, 10))])   # nine clipped points: fewer than k
    n, seen = int(np.searchsorted(c, m + 1)), set()
    for _ in range(600):
        got, band = filtered_count(big[:n], cfg)
        if got == m and band == 0:
            return np.ascontiguousarray(big[:n])
        seen.add(n)
        step = (max(1, abs(m - got)) if m > 65 else 1) * (1 if got <= m or m <= 65 else -1)   # (small m: every prefix in turn)
        n = min(len(big), max(cfg.normal_k, n + step))
        while n in seen:
            n += 1
    raise AssertionError(f"no prefix with {m} filtered points")


def pcl_compute_model(draws, m, cfg):
    """A literal transcription of pcl::RandomSampleConsensus<PointT>::computeModel (sample_consensus/impl/ransac.hpp) with the model's
    getSamples / computeModelCoefficients / countWithinDistance replaced by `draws`, an iterator of (ok, n_inliers); an exhausted
    iterator stands for "the caller's table ran out".  -> (iterations_, skipped_count, index of the accepted draw, ran out)"""
    iterations_ = 0
    n_best_inliers_count = -(2**31 - 1)
    k = 1.0
    log_probability = math.log(1.0 - cfg.probability)
    one_over_indices = 1.0 / float(m)
    skipped_count = 0
    max_skip = cfg.max_iterations * 10
    model_, at = None, -1
    while iterations_ < k and skipped_count < max_skip:
        try:
            ok, n_inliers_count = next(draws)
        except StopIteration:
            return iterations_, skipped_count, (-1 if model_ is None else model_), 1
        at += 1
        if not ok:
            skipped_count += 1
            continue
        if n_inliers_count > n_best_inliers_count:
            n_best_inliers_count = n_inliers_count
            model_ = at
            w = float(n_best_inliers_count) * one_over_indices
            p_no_outliers = 1.0 - (w * w) * w
            p_no_outliers = max(np.finfo(np.float64).eps, p_no_outliers)
            p_no_outliers = min(1.0 - np.finfo(np.float64).eps, p_no_outliers)
            k = log_probability / math.log(p_no_outliers)
        iterations_ += 1
        if iterations_ > cfg.max_iterations:
            break
    return iterations_, skipped_count, (-1 if model_ is None else model_), 0


# ------------------------------------------------------------------ CPU
def test_symbols_are_exported_and_defaults_are_the_nodelets(mods):
    """fails without the feature: the library exports the apdgicp_floor_* entry points"""
    reg, fd, _ = mods
    L = reg.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name) and name in reg.SYMBOLS
    p = fd.default_floor_params()   # initialize_params() (floor_detection_nodelet.cpp:62-70) and radar_graph_slam.launch
    assert (p.tilt_deg, p.sensor_height, p.height_clip_range, p.floor_pts_thresh, p.floor_normal_thresh, p.use_normal_filtering, p.normal_filter_thresh,
            p.floor_tolerance) == (0.0, 2.0, 1.0, 50, 10.0, 1, 20.0, 0.1)
    assert (p.distance_threshold, p.probability, p.max_iterations, p.normal_k) == (0.06, 0.99, 1000, 10)
    assert 1 <= p.n_hypotheses <= 1024
    c = F.Config()
    for name in c.__dataclass_fields__:
        assert getattr(p, name) == getattr(c, name), name


def test_parameter_errors_need_no_device_and_no_gpu_fails_loudly(mods):
    import torch
    reg, fd, _ = mods
    for kw in (dict(normal_k=2), dict(normal_k=65), dict(n_hypotheses=0), dict(n_hypotheses=1025), dict(distance_threshold=0.0), dict(distance_threshold=-1.0),
               dict(floor_normal_thresh=0.0), dict(normal_filter_thresh=-5.0), dict(height_clip_range=0.0), dict(probability=1.0), dict(max_iterations=0)):
        with pytest.raises(reg.ApdgicpError) as e:
            fd.FloorDetector(**kw)
        assert e.value.code == -1, kw
    if not torch.cuda.is_available():
        with pytest.raises(reg.ApdgicpError) as e:
            fd.FloorDetector()
        assert e.value.code == -5


def test_floor_scan_is_deterministic_and_has_its_parts(scene):
    c = scene.floor_scan(4096, 3)
    assert c.shape == (4096, 4) and c.dtype == F32 and np.array_equal(c, scene.floor_scan(4096, 3)) and not np.array_equal(c, scene.floor_scan(4096, 4))
    z = c[:, 2]
    assert 0.45 < (np.abs(z + 2.0) < 0.1).mean() < 0.6 and 0.04 < (z < -2.25).mean() < 0.06 and (z > 0).mean() > 0.1
    t = scene.floor_scan(4096, 3, tilt_deg=5.0, noise=0.0)
    a = np.deg2rad(5.0)
    level_z = -np.sin(a) * t[:, 0] + np.cos(a) * t[:, 2]
    assert 0.45 < (np.abs(level_z + 2.0) < 1e-4).mean() < 0.6


@pytest.mark.parametrize("tilt_deg", [0.0, 5.0])
def test_restatement_recovers_the_plane(scene, tilt_deg):
    scan = scene.floor_scan(4096, 5, tilt_deg=tilt_deg, noise=0.0)
    cfg = F.Config(tilt_deg=tilt_deg)
    st = F.State.initial(cfg)
    r = F.detect(scan, cfg, words_for(cfg.n_hypotheses, 1), st)
    a = math.radians(tilt_deg)
    assert r.detected and st.initialized and r.n_inliers > 1500
    assert np.abs(r.coeffs.astype(np.float64) - np.array([-math.sin(a), 0.0, math.cos(a), 2.0])).max() < 1e-5
    below = scan[:, 2] * math.cos(a) - scan[:, 0] * math.sin(a) < -2.15
    assert below.sum() > 100 and not np.isin(np.flatnonzero(below), r.under_src).any() and len(r.under_src) == len(scan) - below.sum()


def test_replay_is_pcls_sequential_loop():
    rng = np.random.default_rng(7)
    for t in range(200):
        K = int(rng.integers(1, 200))
        m = int(rng.integers(50, 3000))
        cfg = F.Config(max_iterations=int(rng.choice([1, 3, 20, 1000])), probability=float(rng.choice([0.5, 0.99, 0.999])))
        hi = int(rng.choice([3, m // 20 + 3, m // 2, m]))
        n_in = rng.integers(0, hi + 1, K).astype(np.int32)
        bad = rng.random(K) < rng.choice([0.0, 0.1, 0.9, 1.0])
        n_in[bad] = 0
        assert F.replay(n_in, bad, m, cfg) == pcl_compute_model(iter([(not b, int(c)) for b, c in zip(bad, n_in)]), m, cfg), t
    assert F.replay(np.zeros(4, dtype=np.int32), np.zeros(4, dtype=bool), 49, F.Config()) == (0, 0, -1, 0)   # :177, RANSAC never runs


def build_cpp():
    import __graft_entry__ as g
    g.build()
    exe = os.path.join(ROOT, "tests", "cpp", "_build", "test_floor_detection")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    lib_dir = os.path.join(ROOT, "riv-slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "tests", "pcl_shim"), "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "riv-slam_amd", "cpp"), os.path.join(ROOT, "tests", "cpp", "test_floor_detection.cpp"),
                           "-L", lib_dir, "-lapdgicp_hip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-o", exe])
    return exe


def test_cpp_class_compiles():
    out = subprocess.run([build_cpp()], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "compile-only" in out.stdout


# ------------------------------------------------------------------ GPU
def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def cfg_kw(cfg):
    return {k: (int(v) if isinstance(v, bool) else v) for k, v in ((k, getattr(cfg, k)) for k in cfg.__dataclass_fields__)}


def preconditions(scan, cfg, words, state):
    """on the restatement alone: the share of points in the band, no inlier decision within 1 ulp of the threshold"""
    r = F.detect(scan, cfg, words, F.State(state.prev.copy(), state.initialized))
    if r.stat is not None:
        thr = math.cos(cfg.normal_filter_thresh * math.pi / 180.0)
        in_band = np.abs(r.stat.astype(np.float64) - thr) <= BAND
        assert in_band.sum() <= 0.005 * len(r.stat)
    t = F32(cfg.distance_threshold)
    lo, hi = float(np.nextafter(t, F32(0))), float(np.nextafter(t, F32(1)))
    if r.ransac:
        xyz = r.filtered[:, :3]
        for k in np.flatnonzero(~r.bad):
            d = np.abs(F.plane_dist(r.coef[k], xyz)).astype(np.float64)
            assert not ((d >= lo) & (d <= hi)).any()
    return r


def run_and_compare(fd, scan, cfg, words=None, det=None, state=None, device_input=False):
    """one run on the device against the restatement; returns (restatement, result, detector, state)"""
    if words is None:
        words = words_for(cfg.n_hypotheses)
    state = state if state is not None else F.State.initial(cfg)
    pre = preconditions(scan, cfg, words, state)
    det = det if det is not None else fd.FloorDetector(**cfg_kw(cfg))
    cloud = scan
    if device_input:
        import torch
        cloud = torch.from_numpy(scan).cuda()
    r = det.run(cloud, words=words)
    d = det.debug()
    clipped, filtered = det.to_numpy("clipped"), det.to_numpy("filtered")
    assert np.array_equal(d["clip_mask"], pre.clip_mask) and r.n_clipped == len(pre.clipped) and r.n_input == len(scan)
    assert np.array_equal(bits(clipped["xyzi"]), bits(pre.clipped)) and np.array_equal(clipped["index"], pre.clip_src)
    keep = np.isin(pre.clip_src, filtered["index"])
    if pre.stat is not None:
        thr = math.cos(cfg.normal_filter_thresh * math.pi / 180.0)
        err = np.abs(d["normal_stat"].astype(np.float64) - pre.stat.astype(np.float64))
        print(f"floor: n_clipped={len(pre.stat)} normal statistic max err {err.max():.3e}, in band {(np.abs(pre.stat - thr) <= BAND).sum()}")
        assert err.max() <= BAND
        clear = np.abs(pre.stat.astype(np.float64) - thr) > BAND
        assert np.array_equal(keep[clear], pre.nf_keep[clear])
    else:
        assert np.array_equal(keep, pre.nf_keep)
    ref = F.detect(scan, cfg, words, state, nf_keep=keep if cfg.use_normal_filtering else None)
    assert r.n_filtered == len(ref.filtered)
    assert np.array_equal(bits(filtered["xyzi"]), bits(ref.filtered)) and np.array_equal(filtered["index"], ref.filt_src)
    coef, bad, n_in = det.hypotheses()
    assert np.array_equal(d["samples"], ref.samples) and np.array_equal(bad, ref.bad)
    assert np.array_equal(bits(coef), bits(ref.coef)) and np.array_equal(n_in, ref.n_in)
    assert (r.iterations, r.skipped, r.winner, r.table_exhausted) == (ref.iterations, ref.skipped, ref.winner, ref.exhausted)
    assert (bool(r.detected), r.reject_reason, bool(r.ground_initialized)) == (ref.detected, ref.reason, ref.initialized)
    assert np.array_equal(bits(list(r.coeffs)), bits(ref.coeffs)) and np.array_equal(bits(list(r.raw_coeffs)), bits(ref.raw)) and r.n_inliers == ref.n_inliers
    inl, under = det.to_numpy("inliers"), det.to_numpy("under_floor")
    assert np.array_equal(inl["index"], ref.inlier_src) and np.array_equal(bits(inl["xyzi"]), bits(ref.inlier_xyzi))
    assert r.n_under_floor == len(ref.under_src) and np.array_equal(under["index"], ref.under_src) and np.array_equal(bits(under["xyzi"]), bits(ref.under_xyzi))
    for dp, k in ((det.inlier_cloud(), len(ref.inlier_src)), (det.under_floor_filtered(), len(ref.under_src))):
        assert dp.n == k and dp.stride_bytes == 16 and (dp.ptr != 0) == (k > 0)
    return ref, r, det, state


M_ALL = [0, 9, 10, 49, 50, 63, 64, 65, 255, 256, 257, 1023, 1025, 5000]


@pytest.mark.gpu
@pytest.mark.parametrize("m", M_ALL)
def test_sizes_at_the_edges_without_the_normal_filter(mods, m):
    """m filtered points around normal_k (10), floor_pts_thresh (50), the wave (64), the scoring tile (256) and the compaction block (1024)"""
    _, fd, _ = mods
    tilt = 5.0 if m % 2 else 0.0
    scan = scan_with_m(m, False, tilt)
    ref, r, _, _ = run_and_compare(fd, scan, F.Config(tilt_deg=tilt, use_normal_filtering=False), device_input=m % 3 == 1)
    assert r.n_filtered == m and ref.ransac == (m >= 50) and (m < 257 or ref.detected)
    if m == 0:
        det = fd.FloorDetector()
        empty = det.run(np.zeros((0, 4), dtype=F32))
        assert (empty.detected, empty.n_input, empty.n_under_floor, empty.K, empty.winner) == (0, 0, 0, 64, -1) and det.under_floor_filtered().n == 0


@pytest.mark.gpu
@pytest.mark.parametrize("m", M_ALL)
def test_sizes_at_the_edges_with_the_normal_filter(mods, scene, m):
    """the same sizes behind the k-NN epilogue; m = 0: nine clipped points, fewer than k, no search; ~5000: whatever a 24k scan gives"""
    _, fd, _ = mods
    tilt = 0.0 if m % 2 else 5.0
    scan = scan_with_m(m, True, tilt) if m < 5000 else scene.floor_scan(12000, 23, tilt_deg=tilt)
    ref, r, _, _ = run_and_compare(fd, scan, F.Config(tilt_deg=tilt), device_input=m % 3 == 2)
    if m < 5000:
        assert r.n_filtered == m and ref.ransac == (m >= 50)
        assert (r.n_clipped == 9) == (m == 0)
    else:
        assert 4000 < r.n_filtered < 7000 and ref.detected


@pytest.mark.gpu
@pytest.mark.parametrize("tilt_deg", [0.0, 5.0])
@pytest.mark.parametrize("K", [1, 63, 64, 65, 1024])
def test_hypothesis_counts(mods, K, tilt_deg):
    _, fd, _ = mods
    ref, r, _, _ = run_and_compare(fd, scan_with_m(1025, False, tilt_deg), F.Config(tilt_deg=tilt_deg, use_normal_filtering=False, n_hypotheses=K), words_for(K, seed=K))
    assert r.K == K and ref.ransac and (K < 63 or ref.detected) and (K < 1024 or not ref.exhausted)


@pytest.mark.gpu
def test_the_callbacks_memory(mods, scene):
    """no floor, no floor, floor, no floor, reset -- against the restatement, which carries the same state"""
    _, fd, _ = mods
    cfg = F.Config(use_normal_filtering=False)
    nothing, floor = scan_with_m(49, False, 0.0), scene.floor_scan(3000, 31)
    ref, r, det, st = run_and_compare(fd, nothing, cfg)
    assert not ref.detected and list(r.coeffs) == [0, 0, 1, 0] and r.n_under_floor == len(nothing) and not r.ground_initialized
    ref, r, _, _ = run_and_compare(fd, nothing, cfg, det=det, state=st)
    assert not ref.detected and list(r.coeffs) == [0, 0, 1, 0] and r.n_under_floor == len(nothing)
    ref, r, _, _ = run_and_compare(fd, floor, cfg, det=det, state=st, words=words_for(64, 2))
    assert ref.detected and r.ground_initialized and 0.04 * len(floor) < len(floor) - r.n_under_floor < 0.06 * len(floor)
    found = list(r.coeffs)
    ref, r, _, _ = run_and_compare(fd, nothing, cfg, det=det, state=st)
    assert not ref.detected and r.ground_initialized and list(r.coeffs) == found and r.n_under_floor < len(nothing)   # previous coefficients published and used
    det.reset()
    st2 = F.State.initial(cfg)
    ref, r, _, _ = run_and_compare(fd, nothing, cfg, det=det, state=st2)
    assert not r.ground_initialized and list(r.coeffs) == [0, 0, 1, 0] and r.n_under_floor == len(nothing)


def first_words(scan, cfg, cond, tries=60):
    for seed in range(tries):
        w = words_for(cfg.n_hypotheses, 100 + seed)
        if cond(F.detect(scan, cfg, w, F.State.initial(cfg))):
            return w
    raise AssertionError("no table of words with that outcome")


def wall_only_scan():
    """one wall x = 10 m (1 cm thick) from 1 m below the sensor's floor to 3 m above the sensor, clutter above the height band only"""
    rng = np.random.default_rng(33)
    wall = np.stack([10.0 + 0.01 * rng.normal(size=900), rng.uniform(-5, 5, 900), rng.uniform(-3, 3, 900)], axis=1)
    above = np.stack([rng.uniform(2, 40, 300), rng.uniform(-15, 15, 300), rng.uniform(-0.9, 4, 300)], axis=1)
    xyz = np.concatenate([wall, above], axis=0)[rng.permutation(1200)]
    return np.ascontiguousarray(np.concatenate([xyz, rng.uniform(0, 40, (1200, 1))], axis=1).astype(F32))


@pytest.mark.gpu
def test_rejections(mods, scene):
    _, fd, _ = mods
    off = dict(use_normal_filtering=False)
    ref, _, _, _ = run_and_compare(fd, scan_with_m(49, False, 0.0), F.Config(**off))                      # too few points (:177)
    assert ref.reason == F.FEW_POINTS and not ref.ransac
    ref, r, _, _ = run_and_compare(fd, scan_with_m(257, False, 0.0), F.Config(floor_pts_thresh=250, **off))  # too few inliers (:192)
    assert ref.reason == F.FEW_INLIERS and 0 < r.n_inliers < 250 and r.winner >= 0 and any(r.raw_coeffs)
    ref, _, _, _ = run_and_compare(fd, wall_only_scan(), F.Config(**off))                                  # a wall-only scan (:203-208)
    assert ref.reason == F.NOT_HORIZONTAL and abs(ref.raw[2]) < 0.2 and ref.n_inliers > 200
    i = np.arange(64, dtype=np.float64)                                                                  # a collinear-only cloud: every sample is bad
    line = np.stack([2.0 + 0.25 * i, 0.25 * i - 8.0, -2.0 + i / 128.0, i], axis=1).astype(F32)
    ref, r, _, _ = run_and_compare(fd, line, F.Config(**off))
    assert ref.bad.all() and (r.iterations, r.skipped, r.winner, r.table_exhausted, r.reject_reason) == (0, 64, -1, 1, F.NO_MODEL)
    scan = scene.floor_scan(2000, 34)                                                                    # a downward normal is flipped (:211-213)
    cfg = F.Config(n_hypotheses=8)
    for down in (True, False):
        ref, r, _, _ = run_and_compare(fd, scan, cfg, first_words(scan, cfg, lambda e: e.detected and (e.raw[2] < 0) == down))
        assert r.detected and (r.raw_coeffs[2] < 0) == down and r.coeffs[2] > 0.99 and abs(r.coeffs[3] - 2.0) < 0.05


@pytest.mark.gpu
def test_residency_repeatability_and_layouts(mods, scene):
    """under_floor_filtered() as the device input of ScanFilter.run and setInputSource against the host path; two runs are byte-identical;
    host input = device input (run_and_compare's device_input); a strided layout"""
    import ctypes
    import torch
    reg, fd, sf = mods
    scan = scene.floor_scan(6000, 35)
    words = words_for(64, 5)
    det = fd.FloorDetector()
    r1 = det.run(scan, words=words)
    snap = lambda: (bytes(ctypes.string_at(ctypes.addressof(det.result), 96)), {k: det.to_numpy(k) for k in ("filtered", "inliers", "under_floor")}, det.hypotheses())
    a = snap()
    under = a[1]["under_floor"]["xyzi"]
    assert r1.detected and 0 < r1.n_under_floor < len(scan)
    f_dev, f_host = sf.ScanFilter(), sf.ScanFilter()
    n_dev, n_host = f_dev.run(det.under_floor_filtered()), f_host.run(under)
    assert n_dev == n_host > 0 and np.array_equal(bits(f_dev.to_numpy()), bits(f_host.to_numpy()))
    g_dev, g_host = reg.FastAPDGICP(reg.default_params()), reg.FastAPDGICP(reg.default_params())
    g_dev.setInputSource(det.under_floor_filtered())
    g_host.setInputSource(under)
    assert g_dev.n_src == g_host.n_src == r1.n_under_floor and np.array_equal(bits(g_dev.getPoints(0)), bits(g_host.getPoints(0)))
    det.reset()
    det.run(scan, words=words)
    b = snap()
    assert a[0] == b[0] and all(np.array_equal(bits(a[1][k]["xyzi"]), bits(b[1][k]["xyzi"])) and np.array_equal(a[1][k]["index"], b[1][k]["index"]) for k in a[1])
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a[2], b[2]))
    wide = np.full((len(scan), 8), np.nan, dtype=F32)   # a pcl::PointXYZI-like layout: 32 bytes, intensity at 16
    wide[:, :3], wide[:, 4] = scan[:, :3], scan[:, 3]
    for cloud in (wide, torch.from_numpy(wide).cuda()):
        det.reset()
        det.run(cloud, words=words, intensity_column=4)
        c = snap()
        assert a[0] == c[0] and all(np.array_equal(bits(a[1][k]["xyzi"]), bits(c[1][k]["xyzi"])) for k in a[1])
    with pytest.raises(reg.ApdgicpError) as e:
        det.run(scan, words=words[:63])   # too few words
    assert e.value.code == -1
    small = np.zeros(len(scan) - 1, dtype=np.uint8)   # a destination sized for another run is refused, not overrun
    det.run(scan, words=words)
    assert det.L.apdgicp_floor_debug(det.h, small.ctypes.data_as(ctypes.c_void_p), small.size, None, 0, None, 0) == -1 and not small.any()


@pytest.mark.gpu
def test_cpp_class_returns_the_python_paths_record(mods, scene, tmp_path):
    import ctypes
    _, fd, _ = mods
    exe = build_cpp()
    scan = scene.floor_scan(4096, 36)
    path, outp = tmp_path / "scan.bin", tmp_path / "out.bin"
    with open(path, "wb") as fh:
        np.array([len(scan)], dtype=np.int32).tofile(fh)
        scan.tofile(fh)
    out = subprocess.run([exe, str(path), str(outp), "7"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split()[-1] == "1"
    mt = np.random.MT19937()   # std::mt19937 seeded with 7: numpy's generator seeded the same way gives the same 32-bit words
    mt._legacy_seeding(7)
    words = mt.random_raw(32 * 3).astype(np.uint32).reshape(32, 3)
    det = fd.FloorDetector(n_hypotheses=32)
    r = det.run(scan, words=words)
    raw = open(outp, "rb").read()
    assert raw[:96] == bytes(ctypes.string_at(ctypes.addressof(r), 96)) and r.detected
    n_floor = int(np.frombuffer(raw, dtype=np.int32, count=1, offset=96)[0])
    fp = np.frombuffer(raw, dtype=F32, count=4 * n_floor, offset=100).reshape(-1, 4)
    n_under = int(np.frombuffer(raw, dtype=np.int32, count=1, offset=100 + 16 * n_floor)[0])
    uf = np.frombuffer(raw, dtype=F32, count=4 * n_under, offset=104 + 16 * n_floor).reshape(-1, 4)
    assert np.array_equal(bits(fp), bits(det.to_numpy("inliers")["xyzi"])) and np.array_equal(bits(uf), bits(det.to_numpy("under_floor")["xyzi"]))
