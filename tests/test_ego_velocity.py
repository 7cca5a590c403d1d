"""Doppler ego velocity and moving-point removal on the device (riv-slam_amd/ego_velocity.py, csrc/apd_ego.hpp):
rio::RadarEgoVelocityEstimator::estimate (radar_graph_slam/src/radar_ego_velocity_estimator.cpp).

The expected values come from tests/ego_velocity_np.py, a numpy restatement that follows the reference statement by statement in the
operation orders include/apdgicp_hip.h states, fed with the same table of random words.

Bars (GPU): the valid mask, the compacted rows, the selected |v|, the zero-velocity decision, every sampled index, every v_k, every
n_in[k], best_in / best_out, the inlier / outlier index lists and the two clouds with their dopplers: identical / bit for bit.  The final
v and sigma: within 1e-9 * max(1, |ref|_inf) of the restatement's SEQUENTIAL sums (the device adds the <= 2^13 doubles per sum in a
fixed tree; tests/test_scan_filter.py's bar for the same kind of sum), after asserting on the restatement alone that cond(H^T H) < 1e3.
"""
import importlib
import os
import subprocess

import numpy as np
import pytest

import ego_velocity_np as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
NEW_SYMBOLS = ["apdgicp_ego_velocity_default_params", "apdgicp_ego_velocity_create", "apdgicp_ego_velocity_destroy", "apdgicp_ego_velocity_set_params",
               "apdgicp_ego_velocity_hypothesis_count", "apdgicp_ego_velocity_run", "apdgicp_ego_velocity_inliers", "apdgicp_ego_velocity_outliers",
               "apdgicp_ego_velocity_copy", "apdgicp_ego_velocity_hypotheses", "apdgicp_ego_velocity_debug"]
V_SENSOR = (2.0, 0.3, -0.1)


@pytest.fixture(scope="module")
def mods():
    import __graft_entry__ as g
    g.build()
    return (importlib.import_module("riv-slam_amd.registration"), importlib.import_module("riv-slam_amd.ego_velocity"),
            importlib.import_module("riv-slam_amd.scan_filter"))


def words_for(K, S, seed=0):
    return np.random.default_rng(seed).integers(0, 2**32, (K, S), dtype=np.uint32)


def scan_with_m(scene, m, seed=11, **kw):
    """the shortest prefix of a raw doppler scan with exactly m valid rows, plus the invalid points that follow it.  Of the seeds
    seed, seed + 100, ... the first whose valid rows are a well-posed problem (cond(H^T H) of all of them < 500: a handful of rows
    may lie nearly in a plane), so that the 1e-9 bar on v and sigma is a statement about summation order alone."""
    for s in range(seed, seed + 2000, 100):
        big = scene.raw_doppler_scan(max(64, 2 * m + 64), s, **kw)
        valid, rows = E.features(big, E.Config())
        c = np.cumsum(valid)
        assert c[-1] > m
        if m == 0:
            return np.ascontiguousarray(big[~valid][:40])   # points outside the field of view, below min_db, not finite
        n = int(np.searchsorted(c, m + 1))   # the index of valid row number m + 1: everything before it holds exactly m
        H = rows[:n][valid[:n], :3]
        if m < 5 or np.linalg.cond(H.T @ H) < 500.0:
            return np.ascontiguousarray(big[:n])
    raise AssertionError("no well-conditioned scan")


# ------------------------------------------------------------------ CPU
def test_symbols_are_exported_and_defaults_are_the_estimators(mods):
    """fails without the feature: the library exports the apdgicp_ego_velocity_* entry points"""
    reg, ev, _ = mods
    L = reg.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name) and name in reg.SYMBOLS
    p = ev.default_ego_velocity_params()   # radar_ego_velocity_estimator.h:30-60
    assert (p.min_dist, p.max_dist, p.min_db, p.elevation_thresh_deg, p.azimuth_thresh_deg) == (F32(0.1), 400.0, 5.0, 60.0, 120.0)
    assert (p.thresh_zero_velocity, p.allowed_outlier_percentage, p.doppler_velocity_correction_factor) == (F32(0.05), F32(0.30), 1.0)
    assert (p.sigma_zero_velocity_x, p.sigma_zero_velocity_y, p.sigma_zero_velocity_z) == (F32(1.0e-3), F32(3.2e-3), F32(1.0e-2))
    assert (p.max_sigma_x, p.max_sigma_y, p.max_sigma_z) == (F32(0.2),) * 3 and (p.sigma_offset_radar_x, p.sigma_offset_radar_y, p.sigma_offset_radar_z) == (0, 0, 0)
    assert (p.use_cholesky_instead_of_bdcsvd, p.use_ransac, p.N_ransac_points, p.n_hypotheses) == (1, 1, 5, 0)
    assert (p.outlier_prob, p.success_prob, p.inlier_thresh) == (F32(0.05), F32(0.995), 0.5)


def test_ransac_iter_formula_gives_three_at_the_defaults(mods):
    """setRansacIter (radar_ego_velocity_estimator.h:138-143): uint(log(0.005) / log(1 - 0.95^5)) = 3, in the library and in the restatement"""
    _, ev, _ = mods
    assert ev.hypothesis_count(ev.default_ego_velocity_params()) == 3 == E.ransac_iter(E.Config())
    assert ev.hypothesis_count(ev.default_ego_velocity_params(n_hypotheses=1024)) == 1024
    for kw in (dict(outlier_prob=0.2), dict(success_prob=0.9, N_ransac_points=3), dict(outlier_prob=0.3, N_ransac_points=8)):
        assert ev.hypothesis_count(ev.default_ego_velocity_params(**kw)) == E.ransac_iter(E.Config(**kw))


def test_no_gpu_fails_loudly(mods, scene):
    """without a device the class raises (there is no CPU fall-back); parameter errors need no device"""
    import torch
    reg, ev, _ = mods
    with pytest.raises(reg.ApdgicpError) as e:
        ev.EgoVelocityEstimator(use_cholesky_instead_of_bdcsvd=0)
    assert e.value.code == -5
    for kw in (dict(N_ransac_points=2), dict(N_ransac_points=9), dict(n_hypotheses=1025)):
        with pytest.raises(reg.ApdgicpError) as e:
            ev.EgoVelocityEstimator(**kw)
        assert e.value.code == -1
    if not torch.cuda.is_available():
        with pytest.raises(reg.ApdgicpError):
            ev.EgoVelocityEstimator()


def test_raw_doppler_scan_extends_raw_scan(scene):
    c = scene.raw_doppler_scan(4096, 3, V_SENSOR, 0.02)
    assert c.shape == (4096, 5) and c.dtype == F32 and np.array_equal(c, scene.raw_doppler_scan(4096, 3, V_SENSOR, 0.02), equal_nan=True)
    assert np.array_equal(c[:, :4], scene.raw_scan(4096, 3, 0.02), equal_nan=True) and np.isfinite(c[:, 4]).all()
    still = scene.raw_doppler_scan(4096, 3, (0, 0, 0), 0.0)
    assert np.abs(still[:, 4]).max() < 0.15


def test_restatement_recovers_the_sensor_velocity(scene):
    c = scene.raw_doppler_scan(4096, 5, V_SENSOR, 0.0, doppler_noise=0.0)
    est = E.estimate(c, E.Config(), words_for(3, 5))
    assert est.success and not est.zero_velocity and est.m > 3000 and est.cond < 1e3
    assert np.abs(est.v - np.array(V_SENSOR)).max() < 1e-5 and est.sigma_in_bounds
    noisy = E.estimate(scene.raw_doppler_scan(4096, 5, V_SENSOR, 0.0), E.Config(), words_for(3, 5))
    assert np.abs(noisy.v - np.array(V_SENSOR)).max() < 0.02 and (noisy.sigma < 0.01).all()
    still = E.estimate(scene.raw_doppler_scan(4096, 5, (0, 0, 0), 0.02), E.Config(), words_for(3, 5))
    assert still.zero_velocity and still.success and (still.v == 0).all() and 0.9 * still.m < len(still.inlier_rows) <= still.m


def test_sampler_yields_distinct_in_range_rows():
    ext = np.array([0, 1, 2**31 - 1, 2**31, 2**32 - 1, 2**32 - 2, 12345, 7], dtype=np.uint32)
    rng = np.random.default_rng(3)
    for S in (3, 5, 8):
        for m in (S, S + 1, 64):
            tables = [np.full(S, w, dtype=np.uint32) for w in ext] + [ext[:S], ext[::-1][:S]] + list(rng.integers(0, 2**32, (200, S), dtype=np.uint32))
            seen = set()
            for w in tables:
                idx = E.sample(w, S, m)
                assert len(set(idx)) == S and min(idx) >= 0 and max(idx) < m
                seen.update(idx)
            assert seen == set(range(m))   # every row can be drawn
    assert E.sample(np.zeros(5, dtype=np.uint32), 5, 9) == [0, 1, 2, 3, 4] and E.sample(np.array([8, 7, 6, 5, 4], dtype=np.uint32), 5, 9) == [8, 7, 6, 5, 4]


def build_cpp():
    import __graft_entry__ as g
    g.build()
    exe = os.path.join(ROOT, "tests", "cpp", "_build", "test_ego_velocity")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    lib_dir = os.path.join(ROOT, "riv-slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "tests", "pcl_shim"), "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "riv-slam_amd", "cpp"), os.path.join(ROOT, "tests", "cpp", "test_ego_velocity.cpp"),
                           "-L", lib_dir, "-lapdgicp_hip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-o", exe])
    return exe


def test_cpp_class_compiles():
    out = subprocess.run([build_cpp()], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "compile-only" in out.stdout


# ------------------------------------------------------------------ GPU
def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def close(got, ref):
    ref = np.asarray(ref, dtype=np.float64)
    return bool(np.abs(np.asarray(got) - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max()))


OBSERVED = {"v": 0.0, "sigma": 0.0}


def run_and_compare(ev, scan, cfg: E.Config, words=None, device_input=False):
    """one run on the device against the restatement; returns (restatement, result)"""
    K = E.ransac_iter(cfg) if cfg.use_ransac else 0
    S = int(cfg.N_ransac_points)
    if words is None:
        words = words_for(K, S)
    ref = E.estimate(scan, cfg, words)
    kw = {k: getattr(cfg, k) for k in cfg.__dataclass_fields__ if k not in ("use_ransac",)}
    est = ev.EgoVelocityEstimator(use_ransac=int(cfg.use_ransac), **kw)
    cloud = scan
    if device_input:
        import torch
        cloud = torch.from_numpy(scan).cuda()
    r = est.run(cloud, words=words)
    d = est.debug()
    assert r.m == ref.m and r.K == K
    if len(scan):
        assert np.array_equal(d["valid"], ref.valid)                                                  # the mask ...
        assert np.array_equal(bits64(d["rows"]), bits64(ref.rows))                                    # ... the rows, in the compacted order
    assert bool(r.success) == ref.success and bool(r.zero_velocity) == ref.zero_velocity
    if ref.m > 2:
        assert bits(d["selected_abs_v"])[()] == bits(ref.selected_abs_v)[()]
    vk, n_in = est.hypotheses()
    if ref.samples is not None:
        assert np.array_equal(d["samples"], ref.samples)
        assert np.array_equal(bits64(vk), bits64(ref.v_k)) and np.array_equal(n_in, ref.n_in)
        assert (r.best_in, r.best_out) == (ref.best_in, ref.best_out)
    else:
        assert (r.best_in, r.best_out) == (-1, -1)
    for which, rows in (("inliers", ref.inlier_rows), ("outliers", ref.outlier_rows)):
        got = est.to_numpy(which)
        xyzi, dop, src = ref.cloud(scan, "in" if which == "inliers" else "out")
        assert (r.n_inlier if which == "inliers" else r.n_outlier) == len(rows)
        assert np.array_equal(got["row"], rows) and np.array_equal(got["index"], src)
        assert np.array_equal(bits(got["xyzi"]), bits(xyzi)) and np.array_equal(bits(got["doppler"]), bits(dop))
        dp = est.inliers() if which == "inliers" else est.outliers()
        assert dp.n == len(rows) and dp.stride_bytes == 16 and (dp.ptr != 0) == (len(rows) > 0)
    got_v, got_s = np.array(r.v), np.array(r.sigma)
    if ref.success and not ref.zero_velocity:
        assert ref.cond < 1e3                                                                         # (on the restatement alone)
        ev_, es_ = (np.abs(g - q).max() / max(1.0, np.abs(q).max()) for g, q in ((got_v, ref.v), (got_s, ref.sigma)))
        OBSERVED["v"], OBSERVED["sigma"] = max(OBSERVED["v"], ev_), max(OBSERVED["sigma"], es_)
        print(f"ego velocity: m={ref.m} K={K} S={S} rel err v {ev_:.3e} sigma {es_:.3e} (max so far {OBSERVED['v']:.3e} / {OBSERVED['sigma']:.3e}) cond {ref.cond:.1f}")
        assert close(got_v, ref.v) and close(got_s, ref.sigma)
        assert bool(r.sigma_in_bounds) == ref.sigma_in_bounds
    else:
        assert np.array_equal(got_v, ref.v) and np.array_equal(got_s, ref.sigma)
    return ref, r


@pytest.mark.gpu
@pytest.mark.parametrize("m", [0, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4099])
def test_sizes_at_the_edges_of_the_kernels(mods, scene, m):
    """m valid rows around the wave (64), the scoring tile (256) and the compaction block (1024); S - 1 = 4 and S = 5 at the defaults"""
    _, ev, _ = mods
    scan = scan_with_m(scene, m, v_sensor=V_SENSOR, moving_share=0.02)
    ref, r = run_and_compare(ev, scan, E.Config(), device_input=m % 2 == 1)
    assert ref.m == m and ref.success == (m >= 5) and len(scan) >= max(m, 1)
    if m == 0:
        empty = ev.EgoVelocityEstimator().run(np.zeros((0, 5), dtype=F32))
        assert (empty.success, empty.m, empty.n_inlier, empty.K) == (0, 0, 0, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("S", [3, 5, 8])
@pytest.mark.parametrize("K", [1, 3, 64, 65, 1024])
def test_hypothesis_counts_and_sample_sizes(mods, scene, K, S):
    _, ev, _ = mods
    scan = scan_with_m(scene, 1025, seed=12, v_sensor=V_SENSOR, moving_share=0.02)
    ref, _ = run_and_compare(ev, scan, E.Config(n_hypotheses=K, N_ransac_points=S), words_for(K, S, seed=K + S))
    assert ref.success and ref.samples.shape == (K, S)


@pytest.mark.gpu
def test_too_small_scans_for_the_sample(mods, scene):
    """m = S - 1 and m = S for S = 8"""
    _, ev, _ = mods
    for m, ok in ((7, False), (8, True)):
        ref, _ = run_and_compare(ev, scan_with_m(scene, m, v_sensor=V_SENSOR, moving_share=0.0), E.Config(N_ransac_points=8, n_hypotheses=3))
        assert ref.success == ok


@pytest.mark.gpu
def test_standing_still_takes_the_zero_velocity_branch(mods, scene):
    _, ev, _ = mods
    scan = scene.raw_doppler_scan(4096, 21, (0.0, 0.0, 0.0), 0.02)
    ref, r = run_and_compare(ev, scan, E.Config())
    assert ref.zero_velocity and ref.success and 0 < len(ref.inlier_rows) < ref.m and len(ref.outlier_rows) == 0
    assert list(r.sigma) == [float(F32(1.0e-3)), float(F32(3.2e-3)), float(F32(1.0e-2))] and list(r.v) == [0.0, 0.0, 0.0]
    # ... and at 0 % allowed outliers the clamp: the largest |v| decides (a mover: not standing still by that rule)
    ref0, _ = run_and_compare(ev, scan, E.Config(allowed_outlier_percentage=0.0))
    assert not ref0.zero_velocity


def first_seed(scan, cfg, cond, K, S):
    for seed in range(64):
        w = words_for(K, S, seed)
        if cond(E.estimate(scan, cfg, w)):
            return w
    raise AssertionError("no word table with the wanted property among 64 seeds")


@pytest.mark.gpu
def test_few_movers_give_a_true_split(mods, scene):
    _, ev, _ = mods
    scan = scene.raw_doppler_scan(4096, 22, V_SENSOR, 0.02)
    cfg = E.Config()
    words = first_seed(scan, cfg, lambda e: not e.merged and len(e.outlier_rows) > 0, 3, 5)
    ref, r = run_and_compare(ev, scan, cfg, words)
    assert not ref.merged and 0 < len(ref.outlier_rows) <= 0.05 * ref.m and 0.95 * ref.m <= len(ref.inlier_rows) < ref.m
    if ref.best_in == ref.best_out:   # (else the two lists belong to different hypotheses and need not partition the rows)
        assert len(ref.inlier_rows) + len(ref.outlier_rows) == ref.m
    assert np.abs(np.array(r.v) - np.array(V_SENSOR)).max() < 0.02 and r.sigma_in_bounds == 1


@pytest.mark.gpu
def test_many_movers_merge_every_hypothesis(mods, scene):
    _, ev, _ = mods
    scan = scene.raw_doppler_scan(4096, 23, V_SENSOR, 0.20)
    cfg = E.Config(n_hypotheses=16)
    ref, r = run_and_compare(ev, scan, cfg, words_for(16, 5, 1))
    assert ((ref.m - ref.n_in).astype(F32) / F32(ref.m) > 0.05).all() and ref.merged and ref.best_in == 0 and ref.best_out == -1
    assert len(ref.inlier_rows) == ref.m and len(ref.outlier_rows) == 0 and r.n_outlier == 0
    n0 = int(ref.n_in[0])   # inlier-then-outlier order: two ascending runs
    assert (np.diff(ref.inlier_rows[:n0]) > 0).all() and (np.diff(ref.inlier_rows[n0:]) > 0).all() and 0 < n0 < ref.m


@pytest.mark.gpu
def test_best_out_may_come_from_another_hypothesis(mods, scene):
    """a hand-built word table: hypothesis 0 has the most inliers, hypothesis 1 (not merged either) the most outliers"""
    _, ev, _ = mods
    scan = scene.raw_doppler_scan(2048, 24, V_SENSOR, 0.03, doppler_noise=0.15)
    cfg = E.Config(N_ransac_points=3, n_hypotheses=256)
    cand = words_for(256, 3, 5)
    pool = E.estimate(scan, cfg, cand)
    n_out = pool.m - pool.n_in
    keep = np.flatnonzero((n_out.astype(F32) / F32(pool.m)).astype(np.float64) <= 0.05)
    a, b = keep[np.argmin(n_out[keep])], keep[np.argmax(n_out[keep])]
    assert n_out[b] > n_out[a] > 0
    words = np.stack([cand[a], cand[b]])
    ref, r = run_and_compare(ev, scan, E.Config(N_ransac_points=3, n_hypotheses=2), words)
    assert (ref.best_in, ref.best_out) == (0, 1) and len(ref.outlier_rows) == n_out[b] and len(ref.inlier_rows) == pool.m - n_out[a]


@pytest.mark.gpu
def test_without_ransac_every_valid_row_is_an_inlier(mods, scene):
    _, ev, _ = mods
    scan = scene.raw_doppler_scan(4096, 25, V_SENSOR, 0.02)
    ref, r = run_and_compare(ev, scan, E.Config(use_ransac=False))
    assert ref.success and len(ref.inlier_rows) == ref.m and r.K == 0 and r.n_outlier == 0


@pytest.mark.gpu
def test_bad_rows_and_points_outside_the_field_of_view(mods, scene):
    _, ev, _ = mods
    scan = scene.raw_doppler_scan(4096, 26, V_SENSOR, 0.02)
    finite = np.isfinite(scan[:, :3]).all(axis=1)
    az = np.degrees(np.arctan2(scan[:, 1].astype(np.float64), scan[:, 0]))
    snr_ok = scan[:, 3] > 5
    cfg = E.Config(azimuth_thresh_deg=50.0, elevation_thresh_deg=10.0, doppler_velocity_correction_factor=1.03)
    ref, r = run_and_compare(ev, scan, cfg)
    assert (~finite).sum() == 5 and not ref.valid[~finite].any()
    assert (finite & snr_ok & (np.abs(az) > 51)).sum() > 50 and not ref.valid[finite & (np.abs(az) > 51)].any()
    assert 100 < ref.m < finite.sum() - 100 and (~snr_ok & finite).sum() > 100


@pytest.mark.gpu
def test_with_a_device_the_class_is_created_and_runs(mods, scene):
    _, ev, _ = mods
    assert ev.EgoVelocityEstimator().run(scene.raw_doppler_scan(700, 1)).success == 1


@pytest.mark.gpu
def test_bad_arguments(mods, scene):
    import ctypes
    reg, ev, _ = mods
    est = ev.EgoVelocityEstimator(n_hypotheses=8)
    scan = scene.raw_doppler_scan(512, 27)
    r = est.run(scan)
    small = np.zeros(r.m - 1, dtype=np.uint8)   # a destination sized for another run is refused, not overrun
    rc = est.L.apdgicp_ego_velocity_debug(est.h, small.ctypes.data_as(ctypes.c_void_p), small.size, None, 0, None, 0, None)
    assert rc == -1 and not small.any()
    with pytest.raises(reg.ApdgicpError) as e:
        est.run(scan, words=words_for(7, 5))   # too few words for K * S
    assert e.value.code == -1
    with pytest.raises(reg.ApdgicpError):
        est.run(np.ascontiguousarray(scan[:, :4]))   # no doppler column
    assert est.run(scan).success == 1


@pytest.mark.gpu
def test_estimate_filter_and_set_source(mods, scene):
    """:708-815 + setInputSource without the scan leaving the device, against the same steps through host copies"""
    import ctypes
    reg, ev, sf = mods
    tgt, guess = scene.make_pair(4096, 4096, scene.pair_seed(0, 1), "odometry")[1::2]
    raw = scene.raw_doppler_scan(4096, 28, V_SENSOR, 0.02)
    prm = reg.default_params(max_correspondence_distance=2.0, transformation_epsilon=0.01, azimuth_variance_deg=1.0)
    words = first_seed(raw, E.Config(), lambda e: not e.merged and len(e.outlier_rows) > 0, 3, 5)

    def aligned(setter):
        g = reg.FastAPDGICP(prm)
        g.setInputTarget(tgt)
        f = sf.ScanFilter()
        n = setter(g, f)
        assert 0 < n == g.n_src
        T = g.align(guess)
        return f.to_numpy(), T, bytes(ctypes.string_at(ctypes.addressof(g.result), ctypes.sizeof(g.result)))

    est = ev.EgoVelocityEstimator()
    for removal in (True, False):
        def device_path(g, f):
            res, n = ev.estimate_filter_and_set_source(g, raw, est, f, enable_dynamic_object_removal=removal, words=words)
            assert res.success == 1 and 0 < res.n_outlier and 0.95 * res.m <= res.n_inlier < res.m
            return n
        if removal:
            def host_path(g, f):
                n = f.run(est.to_numpy("inliers")["xyzi"])
                g.setInputSource(f.to_numpy())
                return n
        else:
            def host_path(g, f):
                return sf.preprocess_and_set_source(g, np.ascontiguousarray(raw[:, :4]), f)
        c1, T1, r1 = aligned(device_path)
        c2, T2, r2 = aligned(host_path)
        assert np.array_equal(bits(c1), bits(c2)) and np.array_equal(T1, T2) and r1 == r2


@pytest.mark.gpu
def test_cpp_class_matches_the_c_abi(mods, scene, tmp_path):
    _, ev, _ = mods
    exe = build_cpp()
    c = scene.raw_doppler_scan(4096, 29, V_SENSOR, 0.02)
    path, outp = tmp_path / "scan.bin", tmp_path / "out.bin"
    with open(path, "wb") as fh:
        np.array([len(c)], dtype=np.int32).tofile(fh)
        c.tofile(fh)
    out = subprocess.run([exe, str(path), str(outp), "7"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split()[-1] == "same"
