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


def preconditions(scan, cfg, words, state, on_threshold=None):
    """on the restatement alone: the share of points in the band, no inlier decision within 1 ulp of the threshold.  on_threshold (the
    hand-built scans): instead of excluding such decisions, the filtered points whose distance to the WINNING plane lies within 1 fp32
    ulp of the threshold are exactly these rows"""
    r = F.detect(scan, cfg, words, F.State(state.prev.copy(), state.initialized))
    if r.stat is not None:
        thr = math.cos(cfg.normal_filter_thresh * math.pi / 180.0)
        in_band = np.abs(r.stat.astype(np.float64) - thr) <= BAND
        assert in_band.sum() <= 0.005 * len(r.stat)
    t = F32(cfg.distance_threshold)
    lo, hi = float(np.nextafter(t, F32(0))), float(np.nextafter(t, F32(1)))
    if on_threshold is not None:
        d = np.abs(F.plane_dist(r.coef[r.winner], r.filtered[:, :3])).astype(np.float64) if r.winner >= 0 else np.zeros(0)
        assert np.flatnonzero((d >= lo) & (d <= hi)).tolist() == list(on_threshold)
    elif r.ransac:
        xyz = r.filtered[:, :3]
        for k in np.flatnonzero(~r.bad):
            d = np.abs(F.plane_dist(r.coef[k], xyz)).astype(np.float64)
            assert not ((d >= lo) & (d <= hi)).any()
    return r


def same_bits(got, ref, nan_ok=False):
    """bit for bit; with nan_ok a NaN matches a NaN of any sign and payload"""
    got, ref = np.asarray(got, dtype=F32), np.asarray(ref, dtype=F32)
    both_nan = np.isnan(got) & np.isnan(ref) if nan_ok else np.zeros(ref.shape, dtype=bool)
    return got.shape == ref.shape and bool(((bits(got) == bits(ref)) | both_nan).all())


def run_and_compare(fd, scan, cfg, words=None, det=None, state=None, device_input=False, on_threshold=None, nan_ok=False):
    """one run on the device against the restatement; returns (restatement, result, detector, state).  on_threshold: see preconditions.
    nan_ok: a hypothesis's coefficients match where both sides are NaN and are bit-equal elsewhere."""
    if words is None:
        words = words_for(cfg.n_hypotheses)
    state = state if state is not None else F.State.initial(cfg)
    pre = preconditions(scan, cfg, words, state, on_threshold)
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
    assert same_bits(coef, ref.coef, nan_ok) and np.array_equal(n_in, ref.n_in)
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


# ------------------------------------------------------------------ hand-built scans: comparisons at equality, degenerate samples, 1025 blocks
# Every case is (scan, config, words, check, the rows on the distance threshold): `check` holds the assertions on the restatement alone and
# runs in test_hand_built_inputs_are_the_edges_they_claim without a device, and again in front of the device run of its GPU test.
def nxt(x, towards):
    return np.nextafter(F32(x), F32(towards))


def words_to_draw(rows_wanted):
    """the words with which sample() draws exactly these (distinct) rows, in this order"""
    return np.array([[r - sum(1 for t in rows[:i] if t < r) for i, r in enumerate(rows)] for rows in rows_wanted], dtype=np.uint32)


def flat_floor(n, seed, z=-2.0):
    """n points with z exactly z: every plane through three of them is (0, 0, +-1, -+z) without a rounding"""
    g = np.random.default_rng([seed, 0xF2])
    return np.stack([g.uniform(2, 30, n), g.uniform(-10, 10, n), np.full(n, z), g.uniform(0, 40, n)], axis=1).astype(F32)


def pts(rows):
    return np.array([list(r) + [7.0] for r in rows], dtype=F32)


OFF = dict(use_normal_filtering=False)


class Case:
    def __init__(self, scan, cfg, words, check, on_threshold=(), nan_ok=False):
        self.scan, self.cfg, self.words, self.check = np.ascontiguousarray(scan, dtype=F32), cfg, np.asarray(words, dtype=np.uint32), check
        self.how = dict(on_threshold=list(on_threshold), nan_ok=nan_ok)

    def restate(self, state=None):
        state = F.State.initial(self.cfg) if state is None else F.State(state.prev.copy(), state.initialized)
        ref = F.detect(self.scan, self.cfg, self.words, state)
        self.check(ref)
        return ref

    def run(self, fd, det=None, state=None):
        self.restate(state)   # (the edge is asserted before the device is touched)
        return run_and_compare(fd, self.scan, self.cfg, self.words, det=det, state=state, **self.how)


def exact_plane(ref, d):
    """the winner is (0, 0, +-1, +-d) and the published plane (0, 0, 1, d), exactly"""
    return np.abs(ref.raw).tolist() == [0.0, 0.0, 1.0, d] and ref.raw[2] * ref.raw[3] >= 0 and ref.coeffs.tolist() == [0.0, 0.0, 1.0, d] and not np.signbit(ref.coeffs[2])


def height_band_case():
    """plane_clip(+) keeps distance >= 0, plane_clip(-, negative) drops it: [-(h + range), -(h - range)) = [-3, -1).  Non-finite points
    fail both the band and the under-floor clip (0 * inf is NaN), except z = +inf, which the under-floor clip keeps"""
    inf = np.inf
    edge = pts([(5, 1, -3.0), (5, 1, nxt(-3.0, -4)), (5, 1, -1.0), (5, 1, nxt(-1.0, -2)), (np.nan,) * 3, (inf,) * 3, (-inf,) * 3, (5, 1, inf), (5, 1, -inf)])
    scan = np.concatenate([edge, flat_floor(60, 1)], axis=0)
    cfg = F.Config(n_hypotheses=4, **OFF)

    def check(ref):
        assert ref.clip_mask.tolist() == [True, False, False, True] + [False] * 5 + [True] * 60 and len(ref.filtered) == 62
        assert ref.detected and ref.winner == 0 and ref.n_inliers == 60 and exact_plane(ref, 2.0)
        assert ref.under_src.tolist() == [2, 3, 7] + list(range(9, 69))
    return Case(scan, cfg, words_to_draw([(2, 3, 4), (5, 9, 20), (1, 2, 3), (0, 10, 30)]), check)


def distance_threshold_case():
    """distance_threshold = 0.0625 on the exact plane (0, 0, +-1, +-2): |z + 2| == 0.0625 is an outlier (strict <), one fp32 ulp less an inlier"""
    edge = pts([(5, 1, -1.9375), (5, 1, nxt(-1.9375, -2)), (5, 1, -2.0625), (5, 1, nxt(-2.0625, -2))])
    scan = np.concatenate([flat_floor(60, 2), edge], axis=0)
    cfg = F.Config(distance_threshold=0.0625, n_hypotheses=2, **OFF)

    def check(ref):
        d = np.abs(F.plane_dist(ref.raw, ref.filtered[:, :3])).astype(np.float64)
        assert exact_plane(ref, 2.0) and d[60] == 0.0625 == d[62] == cfg.distance_threshold and d[61] == 0.0625 - 2.0**-23 and d[63] == 0.0625 - 2.0**-22
        assert ref.detected and ref.winner == 0 and ref.n_in[0] == 62 == ref.n_inliers and ref.inlier_rows.tolist() == list(range(60)) + [61, 63]
    return Case(scan, cfg, words_to_draw([(0, 1, 2), (3, 60, 62)]), check, on_threshold=[60, 62])


def fp64_comparison_case():
    """the fp32 distance is widened and compared with the DOUBLE 0.06: (double)0.06f = 0.0599999986... < 0.06, so a point at exactly 0.06f
    from the plane z = 0 is an inlier; compared in fp32 (0.06f < 0.06f) it would not be.  Its neighbour above is an outlier either way"""
    t = F32(0.06)
    edge = pts([(5, 1, t), (5, 1, nxt(t, 1)), (5, 1, -t), (5, 1, nxt(-t, -1))])
    scan = np.concatenate([flat_floor(60, 3, 0.0), edge], axis=0)
    cfg = F.Config(sensor_height=0.0, n_hypotheses=2, **OFF)

    def check(ref):
        assert cfg.distance_threshold == 0.06 and float(t) < 0.06 < float(nxt(t, 1)) and not t < F32(0.06)
        d = np.abs(F.plane_dist(ref.raw, ref.filtered[:, :3]))
        assert exact_plane(ref, 0.0) and d.dtype == F32 and d[60] == t == d[62] and d[61] == nxt(t, 1) == d[63] and len(ref.filtered) == 64
        assert ref.detected and ref.winner == 0 and ref.n_in[0] == 62 == ref.n_inliers and ref.inlier_rows.tolist() == list(range(61)) + [62]
    return Case(scan, cfg, words_to_draw([(0, 1, 2), (3, 60, 62)]), check, on_threshold=[60, 61, 62, 63])


def pts_thresh_case(n_floor):
    """n_best < floor_pts_thresh: 50 inliers of 60 filtered points are a floor, 49 are FEW_INLIERS"""
    scan = np.concatenate([flat_floor(n_floor, 4), flat_floor(60 - n_floor, 5, -2.5)], axis=0)
    cfg = F.Config(n_hypotheses=2, **OFF)

    def check(ref):
        assert len(ref.filtered) == 60 >= cfg.floor_pts_thresh == 50 and ref.ransac and ref.winner == 0 and ref.n_in.tolist()[0] == n_floor == ref.n_inliers
        assert ref.n_in[1] < 49 and ref.detected == (n_floor == 50) and ref.reason == (F.OK if n_floor == 50 else F.FEW_INLIERS)
    return Case(scan, cfg, words_to_draw([(0, 1, 2), (n_floor, n_floor + 1, 0)]), check)


def under_floor_case(detecting):
    """plane_clip(prev + (0, 0, 0, floor_tolerance)) keeps distance >= 0: with the exact plane (0, 0, 1, 2) and tolerance 0.125, z == -2.125 is
    kept and its neighbour below removed -- on the detecting scan and, with the remembered plane, on a scan that detects nothing"""
    edge = pts([(5, 1, -2.125), (5, 1, nxt(-2.125, -3)), (5, 1, 0.5)])
    scan = np.concatenate([flat_floor(60, 6), edge], axis=0) if detecting else edge
    cfg = F.Config(floor_tolerance=0.125, n_hypotheses=2, **OFF)

    def check(ref):
        n = len(scan)
        assert float(F32(2.0 + 0.125)) == 2.125 and ref.coeffs.tolist() == [0.0, 0.0, 1.0, 2.0] and ref.initialized
        assert ref.detected == detecting and (detecting or ref.reason == F.FEW_POINTS)
        assert ref.under_src.tolist() == list(range(n - 3)) + [n - 3, n - 1]
    return Case(scan, cfg, words_to_draw([(0, 1, 2), (3, 4, 5)]), check)


def degenerate_samples_case():
    """computeModelCoefficients on samples that are no triangles.  Rows 0 and 1 are the same point.
      (0, 1, 2): p1 == p0, p2 - p0 without a zero: the ratios are (0, 0, -0), all equal: collinear, bad;
      (0, 2, 3): p2 - p0 = (0, 3, 0.5): a division by zero in the test (inf), not collinear: a plane;
      (0, 2, 1): p2 == p0: the ratios are (inf, inf, -inf): PASSES, the cross product is zero: NaN coefficients, no inlier;
      (2, 0, 1): p1 - p0 == p2 - p0: ratios (1, 1, 1): bad;      (0, 3, 1): ratios (NaN, inf, inf): passes, NaN coefficients;
      (10, 20, 30): three floor points: the winner"""
    g = np.random.default_rng(8)
    special = pts([(1, 1, -2), (1, 1, -2), (2, 3, -2.5), (1, 4, -1.5)])
    floor = flat_floor(60, 7)
    floor[:, 2] += (0.002 * g.normal(size=60)).astype(F32)   # (not exactly flat: a flat sample has 0 / 0 among its ratios)
    scan = np.concatenate([special, floor], axis=0)
    cfg = F.Config(n_hypotheses=7, **OFF)
    draws = [(0, 1, 2), (0, 2, 3), (0, 2, 1), (2, 0, 1), (0, 3, 2), (10, 20, 30), (0, 3, 1)]

    def check(ref):
        assert ref.samples.tolist() == [list(d) for d in draws] and len(ref.filtered) == 64
        assert ref.bad.tolist() == [True, False, False, True, False, False, False]
        assert np.isnan(ref.coef[2]).all() and np.isnan(ref.coef[6]).all() and np.isfinite(ref.coef[[1, 4, 5]]).all()
        assert ref.n_in[2] == 0 == ref.n_in[6] and ref.n_in[1] > 0 and ref.n_in[5] > 50
        assert (ref.winner, ref.skipped, ref.iterations, ref.exhausted) == (5, 2, 4, 0) and ref.detected
    return Case(scan, cfg, words_to_draw(draws), check, nan_ok=True)


BIG_N = 1024 * 1024 + 1025


@functools.lru_cache(maxsize=None)
def more_than_1024_blocks_case():
    """1025 blocks of 1024 points and one point: the second trip of the b0 loop of k_scan_bsum and k_floor_emit_scan, with its carries.  A
    tiled floor_scan (every tile with an intensity of its own); under-floor points in the last two blocks"""
    base = scene_mod().floor_scan(4096, 41)
    reps = BIG_N // 4096 + 1
    scan = np.tile(base, (reps, 1))
    scan[:, 3] = np.repeat(np.arange(reps, dtype=F32), 4096)
    scan = np.ascontiguousarray(scan[:BIG_N])
    below = np.array([1024 * 1024, 1024 * 1024 + 4, 1024 * 1024 + 424, BIG_N - 2, BIG_N - 1])
    scan[below, 2] = F32(-5.0)
    cfg = F.Config(n_hypotheses=4, **OFF)

    def check(ref):
        assert len(scan) == BIG_N == 1049601 and (BIG_N + 1023) // 1024 == 1026 and set(below // 1024) == {1024, 1025}
        assert ref.detected and len(ref.filtered) > 1024 * 512 and ref.n_inliers > 1024 * 400 and not ref.bad.any()
        assert not np.isin(below, ref.under_src).any() and np.isin(below - 1, ref.under_src).any() and 0.9 * BIG_N < len(ref.under_src) < 0.96 * BIG_N
        assert ref.inlier_rows[-1] // 1024 >= 512   # (the inlier list's own scan runs over the filtered points: more than 512 blocks of them)
    return Case(scan, cfg, words_for(4, 3), check, on_threshold=[])


HAND_BUILT = {"height-band": height_band_case, "distance-threshold": distance_threshold_case, "fp64-comparison": fp64_comparison_case,
              "pts-thresh-50": lambda: pts_thresh_case(50), "pts-thresh-49": lambda: pts_thresh_case(49), "under-floor-detecting": lambda: under_floor_case(True),
              "degenerate-samples": degenerate_samples_case, "more-than-1024-blocks": more_than_1024_blocks_case}


@pytest.mark.parametrize("name", list(HAND_BUILT))
def test_hand_built_inputs_are_the_edges_they_claim(name):
    """the restatement-only half of every hand-built GPU case below: equalities with ==, literal counts and lists, which rows sit on the threshold"""
    case = HAND_BUILT[name]()
    case.restate()
    preconditions(case.scan, case.cfg, case.words, F.State.initial(case.cfg), case.how["on_threshold"])


def test_under_floor_edge_with_the_remembered_plane():
    """(the second scan of test_under_floor_clip_at_equality, on the restatement: it needs the state the first one leaves)"""
    st = F.State.initial(F.Config(floor_tolerance=0.125, **OFF))
    a, b = under_floor_case(True), under_floor_case(False)
    a.check(F.detect(a.scan, a.cfg, a.words, st))
    b.restate(st)


@pytest.mark.gpu
def test_height_band_at_equality(mods):
    """z == -3 kept, below dropped; z == -1 dropped, below kept; NaN / inf points dropped"""
    height_band_case().run(mods[1])


@pytest.mark.gpu
def test_distance_threshold_at_equality(mods):
    ref, r, _, _ = distance_threshold_case().run(mods[1])
    assert r.n_inliers == 62 and list(r.coeffs) == [0.0, 0.0, 1.0, 2.0]


@pytest.mark.gpu
def test_distance_is_compared_in_double(mods):
    ref, r, _, _ = fp64_comparison_case().run(mods[1])
    assert r.n_inliers == 62


@pytest.mark.gpu
@pytest.mark.parametrize("n_floor", [50, 49])
def test_floor_pts_thresh_on_the_inlier_count(mods, n_floor):
    ref, r, _, _ = pts_thresh_case(n_floor).run(mods[1])
    assert (r.detected, r.n_inliers, r.reject_reason) == ((1, 50, F.OK) if n_floor == 50 else (0, 49, F.FEW_INLIERS))


@pytest.mark.gpu
def test_under_floor_clip_at_equality(mods):
    ref, r, det, st = under_floor_case(True).run(mods[1])
    assert r.detected and r.n_under_floor == 62
    ref, r, _, _ = under_floor_case(False).run(mods[1], det=det, state=st)
    assert not r.detected and r.ground_initialized and r.n_under_floor == 2 and list(r.coeffs) == [0.0, 0.0, 1.0, 2.0]


@pytest.mark.gpu
def test_degenerate_samples(mods):
    ref, r, det, _ = degenerate_samples_case().run(mods[1])
    coef, bad, n_in = det.hypotheses()
    assert np.isnan(coef[[2, 6]]).all() and bad.tolist() == [True, False, False, True, False, False, False] and (r.winner, r.skipped) == (5, 2)


@pytest.mark.gpu
def test_more_than_1024_blocks(mods):
    ref, r, _, _ = more_than_1024_blocks_case().run(mods[1])
    assert r.detected and r.n_input == BIG_N and r.n_filtered > 1024 * 512
