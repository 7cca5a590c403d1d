"""Doppler ego velocity and moving-point removal on the device (riv-slam_amd/ego_velocity.py, csrc/apd_ego.hpp):
rio::RadarEgoVelocityEstimator::estimate (radar_graph_slam/src/radar_ego_velocity_estimator.cpp).

The expected values come from tests/ego_velocity_np.py, a numpy restatement that follows the reference statement by statement in the
operation orders include/apdgicp_hip.h states, fed with the same table of random words.

Bars (GPU): the valid mask, the compacted rows, the selected |v|, the zero-velocity decision, every sampled index, every v_k, every
n_in[k], best_in / best_out, the inlier / outlier index lists and the two clouds with their dopplers: identical / bit for bit.  The final
v and sigma: within 1e-9 * max(1, |ref|_inf) of the restatement's SEQUENTIAL sums (the device adds the <= 2^13 doubles per sum in a
fixed tree; tests/test_scan_filter.py's bar for the same kind of sum), after asserting on the restatement alone that cond(H^T H) < 1e3.
"""
import functools
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


def same_bits(got, ref, nan_ok=False):
    """bit for bit; with nan_ok a NaN matches a NaN of any sign and payload (those are the arithmetic unit's, not the project's, to pin)"""
    got, ref = np.asarray(got), np.asarray(ref)
    if got.shape != ref.shape:
        return False
    view = bits64 if ref.dtype == np.float64 else bits
    both_nan = np.isnan(got) & np.isnan(ref) if nan_ok else np.zeros(ref.shape, dtype=bool)
    return bool(((view(got) == view(ref)) | both_nan).all())


def params_of(cfg: E.Config):
    kw = {k: getattr(cfg, k) for k in cfg.__dataclass_fields__ if k not in ("use_ransac",)}
    return dict(use_ransac=int(cfg.use_ransac), **kw)


def run_and_compare(ev, scan, cfg: E.Config, words=None, device_input=False, est=None, nan_ok=False, finite_sigma=True, ref=None):
    """one run on the device against the restatement; returns (restatement, result).  est: an estimator that already holds cfg (default: a
    new one).  nan_ok: the doppler of a row and of an emitted point match where both sides are NaN and are bit-equal elsewhere.
    finite_sigma = False: a fit without a degree of freedom -- sigma is not finite on either side and nothing tighter is asked of it.
    ref: the restatement of exactly this run, when the caller has it already."""
    K = E.ransac_iter(cfg) if cfg.use_ransac else 0
    S = int(cfg.N_ransac_points)
    if words is None:
        words = words_for(K, S)
    if ref is None:
        ref = E.estimate(scan, cfg, words)
    if est is None:
        est = ev.EgoVelocityEstimator(**params_of(cfg))
    cloud = scan
    if device_input:
        import torch
        cloud = torch.from_numpy(scan).cuda()
    r = est.run(cloud, words=words)
    d = est.debug()
    assert r.m == ref.m and r.K == K
    if len(scan):
        assert np.array_equal(d["valid"], ref.valid)                                                  # the mask ...
        assert same_bits(d["rows"], ref.rows, nan_ok)                                                 # ... the rows, in the compacted order
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
        assert np.array_equal(bits(got["xyzi"]), bits(xyzi)) and same_bits(got["doppler"], dop, nan_ok)
        dp = est.inliers() if which == "inliers" else est.outliers()
        assert dp.n == len(rows) and dp.stride_bytes == 16 and (dp.ptr != 0) == (len(rows) > 0)
    got_v, got_s = np.array(r.v), np.array(r.sigma)
    if ref.success and not ref.zero_velocity:
        assert ref.cond < 1e3                                                                         # (on the restatement alone)
        with np.errstate(invalid="ignore"):
            ev_, es_ = (np.abs(g - q).max() / max(1.0, np.abs(q).max()) for g, q in ((got_v, ref.v), (got_s, ref.sigma)))
        OBSERVED["v"], OBSERVED["sigma"] = max(OBSERVED["v"], ev_), max(OBSERVED["sigma"], es_)
        print(f"ego velocity: m={ref.m} K={K} S={S} rel err v {ev_:.3e} sigma {es_:.3e} (max so far {OBSERVED['v']:.3e} / {OBSERVED['sigma']:.3e}) cond {ref.cond:.1f}")
        assert close(got_v, ref.v)
        if finite_sigma:
            assert close(got_s, ref.sigma)
        else:
            assert not np.isfinite(ref.sigma).any() and not np.isfinite(got_s).any() and not ref.sigma_in_bounds
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


# ------------------------------------------------------------------ hand-built scans: comparisons at equality, fixed ranks, reused handles
# Every case is (scan, config, words, check): `check` holds the assertions on the restatement alone -- the equality that makes the case an
# edge, the literal ranks and counts -- and runs in test_hand_built_inputs_are_the_edges_they_claim without a device, and again in front
# of the device run of the GPU test that uses the case.
def nxt(x, towards):
    return np.nextafter(F32(x), F32(towards))


def doppler_of(xyz, v):
    """what a sensor moving with v measures on static points: -(unit direction . v), rounded to fp32"""
    p = np.asarray(xyz, dtype=F32).astype(np.float64)
    return (-(p @ np.asarray(v, dtype=np.float64)) / np.sqrt((p * p).sum(axis=1))).astype(F32)


def static_rows(n, seed, v=V_SENSOR):
    """n valid static points spread over +-57 deg azimuth, +-40 deg elevation, 2 .. 60 m: [n, 5] {x, y, z, intensity, doppler}"""
    g = np.random.default_rng([seed, 0xE6])
    az, el, r = g.uniform(-1.0, 1.0, n), g.uniform(-0.7, 0.7, n), g.uniform(2.0, 60.0, n)
    xyz = (np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], axis=1) * r[:, None]).astype(F32)
    return np.ascontiguousarray(np.concatenate([xyz, g.uniform(10.0, 30.0, (n, 1)).astype(F32), doppler_of(xyz, v)[:, None]], axis=1), dtype=F32)


def with_abs_v(scan, absv, seed):
    """the scan with dopplers of the given |v| (factor 1: v = -doppler exactly), shuffled over the rows, with mixed signs"""
    g = np.random.default_rng([seed, 0xAB])
    absv = np.asarray(absv, dtype=F32)
    out = scan.copy()
    out[:, 4] = absv[g.permutation(len(absv))] * np.where(g.random(len(absv)) < 0.5, F32(-1), F32(1))
    return out


def words_to_draw(rows_wanted):
    """the words with which sample() draws exactly these (distinct) rows, in this order"""
    out = []
    for rows in rows_wanted:
        out.append([r - sum(1 for t in rows[:i] if t < r) for i, r in enumerate(rows)])
    return np.array(out, dtype=np.uint32)


class Case:
    def __init__(self, scan, cfg, check, words=None, **how):
        K = E.ransac_iter(cfg) if cfg.use_ransac else 0
        self.scan, self.cfg, self.check, self.how = np.ascontiguousarray(scan, dtype=F32), cfg, check, how
        self.words = words if words is not None else words_for(K, int(cfg.N_ransac_points))

    def restate(self):
        ref = E.estimate(self.scan, self.cfg, self.words)
        self.check(ref)
        return ref

    def run(self, ev, **kw):
        ref = self.restate()   # (the edge is asserted before the device is touched)
        return run_and_compare(ev, self.scan, self.cfg, self.words, ref=ref, **self.how, **kw)


def gate_case(factor):
    """min_dist, max_dist and min_db at equality (strict comparisons: equality is invalid), the fp32 neighbours on either side"""
    x, y = F32(0.1), F32(320.0)
    edge = [[nxt(x, 0), 0, 0, 20], [x, 0, 0, 20], [nxt(x, 1), 0, 0, 20],
            [240, nxt(y, 0), 0, 20], [240, y, 0, 20], [240, nxt(y, 400), 0, 20],
            [3, 1, 0.5, nxt(5, 0)], [3, 1, 0.5, 5.0], [3, 1, 0.5, nxt(5, 6)]]
    edge = np.array(edge, dtype=F32)
    edge = np.concatenate([edge, doppler_of(edge[:, :3], V_SENSOR)[:, None]], axis=1)
    scan = np.concatenate([edge, static_rows(12, 40)], axis=0)
    cfg = E.Config(doppler_velocity_correction_factor=factor)

    def check(ref):
        p = scan[:, :3].astype(np.float64)
        r = np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2])
        assert r[1] == cfg.f("min_dist") and r[4] == 400.0 == cfg.f("max_dist") and scan[7, 3] == F32(cfg.min_db)
        assert r[0] < r[1] < r[2] and r[3] < r[4] < r[5] and scan[6, 3] < scan[7, 3] < scan[8, 3]
        assert ref.valid.tolist() == [False, False, True, True, False, False, False, False, True] + [True] * 12
        assert ref.m == 15 and ref.success and not ref.zero_velocity and ref.cond < 1e3
        assert np.array_equal(bits(ref.rows[:, 3]), bits(-scan[ref.src, 4] * F32(factor)))
    return Case(scan, cfg, check)


RANKS = [(10, 0.30, 6), (20, 0.30, 13), (100, 0.30, 69), (1030, 0.30, 720), (20, 1.0, 0), (1030, 1.0, 0)]


def rank_case(m, allowed, n0):
    """n0 = m * (1.0 - allowed_outlier_percentage) with the FLOAT member widened: 1.0 - 0.30f = 0.69999998..., so 6 / 13 / 69 and not the
    7 / 14 / 70 of 1.0 - 0.3; strictly increasing |v| make the rank visible in the selected value"""
    ladder = (F32(1.0) + np.arange(m, dtype=F32) / F32(1024.0)).astype(F32)
    scan = with_abs_v(static_rows(m, 41), ladder, m)
    cfg = E.Config(allowed_outlier_percentage=allowed)

    def check(ref):
        assert (np.diff(ladder) > 0).all() and np.array_equal(np.sort(np.abs(ref.rows[:, 3].astype(F32))), ladder)
        assert ref.m == m and ref.n0 == n0 == int(m * (1.0 - float(F32(allowed))))
        assert bits(ref.selected_abs_v)[()] == bits(ladder[n0])[()] and not ref.zero_velocity
        if allowed == 0.30 and m <= 100:
            assert int(m * (1.0 - 0.3)) == n0 + 1   # (what a double 0.3 would give)
    return Case(scan, cfg, check)


def zero_threshold_case(lowered):
    """m = 20, rank 13.  The rank-13 |v| is exactly thresh_zero_velocity = 0.05f: not standing still (strict <).  Lowered by one ulp: standing
    still, and the three rows whose |v| == 0.05f are not in the inlier list (strict < there too): 13 + 1 = 14 rows"""
    t = F32(0.05)
    absv = [F32(0.001) * F32(i + 1) for i in range(13)] + [nxt(t, 0) if lowered else t] + [t, t, t] + [F32(0.2), F32(0.3), F32(0.4)]
    scan = with_abs_v(static_rows(20, 42), absv, 7)

    def check(ref):
        av = np.abs(ref.rows[:, 3].astype(F32))
        assert ref.m == 20 and ref.n0 == 13 and (av == t).sum() == (3 if lowered else 4) and (av < t).sum() == (14 if lowered else 13)
        assert bits(ref.selected_abs_v)[()] == bits(nxt(t, 0) if lowered else t)[()] and bits(F32(E.Config().thresh_zero_velocity))[()] == bits(t)[()]
        assert ref.zero_velocity == lowered and ref.success
        if lowered:
            assert len(ref.inlier_rows) == 14 and not (av[ref.inlier_rows] == t).any() and len(ref.outlier_rows) == 0
        else:
            assert ref.cond < 1e3 and len(ref.inlier_rows) == 20
    return Case(scan, E.Config(), check)


RADIX_KINDS = ["equal", "run", "last_byte", "last_two_bytes", "last_three_bytes", "specials_denormal", "specials_zero"]


def radix_case(kind, m):
    """the four 8-bit passes of the selection: ties everywhere, ties across the rank, keys that agree in their upper 3 / 2 / 1 bytes, and
    +-0, denormals and infinities (standing still: the rank falls on a denormal or on a zero, the infinite rows are no inliers)"""
    g = np.random.default_rng([m, RADIX_KINDS.index(kind)])
    n0 = int(m * (1.0 - float(F32(0.30))))
    special = kind.startswith("specials")
    if kind == "equal":
        absv = np.full(m, 1.5, dtype=F32)
    elif kind == "run":
        absv = (F32(1.0) + np.arange(m, dtype=F32) / F32(4096.0)).astype(F32)
        absv[n0 - 5:n0 + 6] = absv[n0 - 5]
    elif special:
        n_zero = int((0.8 if kind == "specials_zero" else 0.4) * m)
        n_den = int(0.15 * m) if kind == "specials_zero" else int(0.45 * m)
        den = g.integers(1, 0x00800000, n_den, dtype=np.uint32).view(F32)
        rest = g.uniform(0.5, 2.0, m - n_zero - n_den - 2).astype(F32)
        absv = np.concatenate([np.zeros(n_zero, dtype=F32), den, rest, np.array([np.inf, np.inf], dtype=F32)])
    else:
        low = {"last_byte": 8, "last_two_bytes": 16, "last_three_bytes": 24}[kind]
        absv = ((np.uint32(0x3FC00000) if low < 24 else np.uint32(0x3F000000)) | g.integers(0, 2**low, m, dtype=np.uint32)).astype(np.uint32).view(F32)
    scan = with_abs_v(static_rows(m, 43), absv, m)
    if special:
        scan[np.flatnonzero(np.isinf(scan[:, 4])), 4] = np.array([np.inf, -np.inf], dtype=F32)
    want = np.sort(absv.view(np.uint32))[n0]

    def check(ref):
        assert ref.m == m and ref.n0 == n0 and bits(ref.selected_abs_v)[()] == want
        key = np.abs(ref.rows[:, 3].astype(F32)).view(np.uint32)
        if kind == "equal":
            assert (key == want).all()
        if kind == "run":
            assert (key == want).sum() == 11 and (key < want).sum() == n0 - 5
        if kind == "last_byte":
            assert ((key >> 8) == (want >> 8)).all() and len(np.unique(key & 255)) > 200
        if kind == "last_two_bytes":
            assert ((key >> 16) == (want >> 16)).all() and len(np.unique((key >> 8) & 255)) > 200
        if kind == "last_three_bytes":
            assert ((key >> 24) == (want >> 24)).all() and len(np.unique((key >> 16) & 255)) > 200
        if special:
            v = ref.rows[:, 3]
            assert (np.signbit(v) & (v == 0)).any() and (~np.signbit(v) & (v == 0)).any() and np.isposinf(v).any() and np.isneginf(v).any()
            assert (want == 0) == (kind == "specials_zero") and want < 0x00800000 and ref.zero_velocity
            assert len(ref.inlier_rows) == (key < bits(F32(0.05))[()]).sum() < m - 2 and not np.isinf(v[ref.inlier_rows]).any()
        else:
            assert not ref.zero_velocity and ref.cond < 1e3
    return Case(scan, E.Config(), check)


def nonfinite_doppler_case(moving):
    """rows whose doppler is NaN / +-inf pass the gate (it does not read the doppler).  Standing still: the NaN sorts behind everything, the
    rank-n0 |v| is still small, and |NaN| < thresh, |inf| < thresh are false.  Moving: no sample draws such a row, so it fails
    |y - H v| < inlier_thresh of every hypothesis: an outlier of an unmerged best_in, and the final fit is finite"""
    bad = np.array([np.nan, np.inf, -np.inf, -np.nan, np.inf], dtype=F32)
    if not moving:
        scan = static_rows(65, 44, (0.0, 0.0, 0.0))
        scan[:, 4] = np.random.default_rng(44).uniform(-0.02, 0.02, 65).astype(F32)
        at = np.array([3, 17, 18, 40, 64])
        scan[at, 4] = bad
        words = None
    else:
        scan = static_rows(200, 45)
        at = np.array([0, 77, 78, 150, 199])
        scan[at, 4] = bad
        words = first_seed(scan, E.Config(), lambda e: not e.merged and not np.isin(e.samples, at).any() and np.isfinite(e.v_k).all(), 3, 5)

    def check(ref):
        assert ref.m == len(scan) and ref.valid.all() and np.array_equal(np.flatnonzero(~np.isfinite(ref.rows[:, 3])), at)
        assert ref.zero_velocity == (not moving) and ref.success
        if not moving:
            assert ref.n0 == 45 and ref.selected_abs_v < 0.02 and len(ref.inlier_rows) == 60 and not np.isin(at, ref.inlier_rows).any()
        else:
            assert not np.isin(ref.samples, at).any() and not ref.merged and (ref.n_in == 195).all()
            assert np.array_equal(ref.outlier_rows, at) and len(ref.inlier_rows) == 195 and np.isfinite(ref.v).all() and np.isfinite(ref.sigma).all()
            assert ref.cond < 1e3 and np.abs(ref.v - np.array(V_SENSOR)).max() < 1e-5
    return Case(scan, E.Config(), check, words, nan_ok=True)


def inlier_threshold_case():
    """|y - H v_k| == inlier_thresh, in exact arithmetic.  The sample is the three axis rows, whose normalised rows are the unit vectors, with
    the dopplers of v = (2, 0.25, -0.5): H^T H = I, v_k = v without a rounding.  Two more axis rows have y - (H v) = +0.5 and -0.5
    exactly (outliers: strict <), two their fp32 neighbours inside (inliers).  3 + 2 + 40 = 45 inliers, 2 of 47 outliers: unmerged"""
    v = (2.0, 0.25, -0.5)
    axis = [[4, 0, 0, 20, -2.0], [0, 8, 0, 20, -0.25], [0, 0, 2, 20, 0.5],
            [16, 0, 0, 20, -2.5], [16, 0, 0, 20, -nxt(2.5, 0)], [0, 0, 4, 20, 1.0], [0, 0, 4, 20, -nxt(-1.0, 0)]]
    scan = np.concatenate([np.array(axis, dtype=F32), static_rows(40, 46, v)], axis=0)
    cfg = E.Config(elevation_thresh_deg=91.0, N_ransac_points=3, n_hypotheses=2)

    def check(ref):
        assert ref.m == 47 and ref.valid.all() and ref.samples.tolist() == [[0, 1, 2], [0, 1, 2]]
        assert np.array_equal(ref.rows[:3, :3], np.eye(3)) and ref.v_k.tolist() == [list(v), list(v)]
        err = E.abs_err(ref.rows, ref.v_k[0])
        assert err[3] == 0.5 == err[5] == cfg.f("inlier_thresh") and err[4] == 0.5 - 2.0**-22 and err[6] == 0.5 - 2.0**-24 and (err[:3] == 0).all()
        assert ref.n_in.tolist() == [45, 45] and ref.outlier_rows.tolist() == [3, 5] and not ref.merged and (ref.best_in, ref.best_out) == (0, 0)
        assert len(ref.inlier_rows) == 45 and ref.cond < 1e3
    return Case(scan, cfg, check, words_to_draw([[0, 1, 2], [0, 1, 2]]))


FIVE_PERCENT = [(20, 1, True), (1280, 64, True), (21, 1, False), (1280, 63, False)]


def five_percent_case(m, movers, merged):
    """float(out) / (in + out) > 0.05 is an fp32 quotient compared with a double: at exactly one outlier in twenty it is 0.05f, which is
    larger than 0.05, so the hypothesis IS merged (a division in double would leave it alone).  The samples avoid the movers"""
    scan = static_rows(m, 47 + m)
    at = np.arange(m // 2 + 2, m // 2 + 2 + movers)
    scan[at, 4] += F32(5.0)
    words = np.array([[0, 0, 0, 0, 0], [1, 2, 3, 4, 5], [5, 4, 3, 2, 1]], dtype=np.uint32)

    def check(ref):
        q = F32(movers) / F32(m)
        assert ref.m == m and ref.samples.max() < at[0] and (ref.n_in == m - movers).all()
        if merged:
            assert bits(q)[()] == bits(F32(0.05))[()] and float(q) > 0.05 and not movers / m > 0.05
            assert ref.merged and (ref.best_in, ref.best_out) == (0, -1) and len(ref.outlier_rows) == 0
            assert np.array_equal(ref.inlier_rows, np.concatenate([np.setdiff1d(np.arange(m), at), at]))
        else:
            assert float(q) < 0.05 and not ref.merged and (ref.best_in, ref.best_out) == (0, 0)
            assert np.array_equal(ref.outlier_rows, at) and np.array_equal(ref.inlier_rows, np.setdiff1d(np.arange(m), at))
        assert ref.cond < 1e3
    return Case(scan, E.Config(), check, words)


def no_ransac_case(m):
    """use_ransac = 0 at m = 4 (one degree of freedom) and m = 3 (none: e^T e / 0, sigma is inf or NaN and out of bounds)"""
    az, el, r = np.array([-0.8, 0.1, 0.9, 0.3])[:m], np.array([0.5, -0.6, 0.2, -0.1])[:m], np.array([5.0, 9.0, 14.0, 20.0])[:m]
    xyz = (np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], axis=1) * r[:, None]).astype(F32)
    scan = np.concatenate([xyz, np.full((m, 1), 20, dtype=F32), doppler_of(xyz, V_SENSOR)[:, None]], axis=1)
    scan[m - 1, 4] += F32(0.01)

    def check(ref):
        assert ref.m == m and ref.success and not ref.zero_velocity and ref.samples is None and ref.inlier_rows.tolist() == list(range(m))
        assert ref.cond < 1e3 and np.abs(ref.v - np.array(V_SENSOR)).max() < 0.1
        if m == 3:
            assert not np.isfinite(ref.sigma).any() and not ref.sigma_in_bounds
        else:
            assert np.isfinite(ref.sigma).all()
    return Case(scan, E.Config(use_ransac=False), check, finite_sigma=m > 3)


BIG_N = 1024 * 1024 + 1025


@functools.lru_cache(maxsize=None)
def more_than_1024_blocks_case():
    """1025 blocks of 1024 rows and one row: the second trip of the b0 loop of k_scan_bsum and k_ego_emit_scan, with its carries.  A tiled
    static scene; three rows fail the gate, five movers sit in the last two blocks of points (valid rows: on either side of the second trip's first block)"""
    base = static_rows(4096, 48)
    scan = np.ascontiguousarray(np.tile(base, (BIG_N // 4096 + 1, 1))[:BIG_N])
    gated = np.array([5, 1024 * 500 + 3, BIG_N - 2000])
    scan[gated, 3] = F32(1.0)
    movers = np.array([1024 * 1024, 1024 * 1024 + 4, 1024 * 1024 + 424, BIG_N - 2, BIG_N - 1])
    scan[movers, 4] += F32(5.0)
    cfg = E.Config()

    def check(ref):
        assert len(scan) == BIG_N == 1049601 and (BIG_N + 1023) // 1024 == 1026 and ref.m == BIG_N - 3 and not ref.valid[gated].any()
        assert set(movers // 1024) == {1024, 1025} and set(ref.outlier_rows // 1024) == {1023, 1024}   # (blocks of points, blocks of valid rows)
        assert not ref.merged and (ref.n_in == ref.m - 5).all() and np.array_equal(ref.src[ref.outlier_rows], movers) and ref.cond < 1e3
        assert len(ref.inlier_rows) == BIG_N - 8 and ref.success and not ref.zero_velocity
    return Case(scan, cfg, check, words_for(3, 5, 2))


def hand_built_cases():
    yield from ((f"gate-{f}", lambda f=f: gate_case(f)) for f in (1.0, 1.03))
    yield from ((f"rank-{m}-{a}", lambda m=m, a=a, n0=n0: rank_case(m, a, n0)) for m, a, n0 in RANKS)
    yield from ((f"zero-threshold-{'below' if low else 'at'}", lambda low=low: zero_threshold_case(low)) for low in (False, True))
    yield from ((f"radix-{kind}-{m}", lambda kind=kind, m=m: radix_case(kind, m)) for kind in RADIX_KINDS for m in (700, 1500))
    yield from ((f"nonfinite-doppler-{'moving' if mv else 'still'}", lambda mv=mv: nonfinite_doppler_case(mv)) for mv in (False, True))
    yield "inlier-threshold", inlier_threshold_case
    yield from ((f"five-percent-{m}-{k}", lambda m=m, k=k, mg=mg: five_percent_case(m, k, mg)) for m, k, mg in FIVE_PERCENT)
    yield from ((f"no-ransac-{m}", lambda m=m: no_ransac_case(m)) for m in (3, 4))
    yield "more-than-1024-blocks", more_than_1024_blocks_case


HAND_BUILT = dict(hand_built_cases())


@pytest.mark.parametrize("name", list(HAND_BUILT))
def test_hand_built_inputs_are_the_edges_they_claim(name):
    """the restatement-only half of every hand-built GPU case below: equalities with ==, literal ranks and counts, cond < 1e3"""
    HAND_BUILT[name]().restate()


def test_words_to_draw_inverts_the_sampler():
    for rows in ([0, 1, 2], [2, 0, 1], [7, 3, 5, 0, 6], [4, 3, 2, 1, 0], [9, 8, 0, 1, 5, 4, 2, 7]):
        assert E.sample(words_to_draw([rows])[0], len(rows), 10) == rows


@pytest.mark.gpu
@pytest.mark.parametrize("factor", [1.0, 1.03])
def test_gate_comparisons_at_equality(mods, factor):
    """r > min_dist, r < max_dist, intensity > min_db: equality is invalid, the fp32 neighbour inside is valid; -doppler * factor in fp32"""
    gate_case(factor).run(mods[1])


@pytest.mark.gpu
@pytest.mark.parametrize("m,allowed,n0", RANKS)
def test_rank_of_the_zero_velocity_test(mods, m, allowed, n0):
    """n0 = 6 / 13 / 69 / 720 (1.0 - 0.30f, not 1.0 - 0.3) and 0 at 100 %: the selected |v| is that rung of a ladder of distinct values"""
    rank_case(m, allowed, n0).run(mods[1])


@pytest.mark.gpu
@pytest.mark.parametrize("lowered", [False, True])
def test_thresh_zero_velocity_at_equality(mods, lowered):
    """|v|[n0] == 0.05f is not standing still; one ulp less is, and rows with |v| == 0.05f are then no inliers (14 rows)"""
    ref, r = zero_threshold_case(lowered).run(mods[1])
    assert r.zero_velocity == int(lowered) and r.n_inlier == (14 if lowered else 20)


@pytest.mark.gpu
@pytest.mark.parametrize("m", [700, 1500])
@pytest.mark.parametrize("kind", RADIX_KINDS)
def test_radix_selection_edges(mods, kind, m):
    """m below and above the block's 1024 lanes; the selected |v| bit for bit"""
    radix_case(kind, m).run(mods[1])


@pytest.mark.gpu
@pytest.mark.parametrize("moving", [False, True])
def test_non_finite_doppler(mods, moving):
    ref, r = nonfinite_doppler_case(moving).run(mods[1])
    assert np.isfinite(np.array(r.v)).all() and np.isfinite(np.array(r.sigma)).all() and r.n_outlier == (5 if moving else 0)


@pytest.mark.gpu
def test_inlier_threshold_at_equality(mods):
    """|y - H v| == 0.5 exactly is an outlier, one fp32 ulp less an inlier: n_in = 45 of 47"""
    ref, r = inlier_threshold_case().run(mods[1])
    assert (r.n_inlier, r.n_outlier) == (45, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("m,movers,merged", FIVE_PERCENT)
def test_five_percent_rule_at_one_in_twenty(mods, m, movers, merged):
    """out / m == 0.05f > 0.05: merged at 1 / 20 and 64 / 1280, unmerged at 1 / 21 and 63 / 1280"""
    ref, r = five_percent_case(m, movers, merged).run(mods[1])
    assert (r.n_inlier, r.n_outlier) == ((m, 0) if merged else (m - movers, movers))


@pytest.mark.gpu
@pytest.mark.parametrize("m", [3, 4])
def test_without_ransac_at_the_smallest_fits(mods, m):
    ref, r = no_ransac_case(m).run(mods[1])
    assert r.success == 1 and r.n_inlier == m and (m > 3 or r.sigma_in_bounds == 0)


@pytest.mark.gpu
def test_more_than_1024_blocks(mods):
    ref, r = more_than_1024_blocks_case().run(mods[1])
    assert r.m == BIG_N - 3 and r.n_outlier == 5 and r.n_inlier == BIG_N - 8


def snapshot(est):
    """everything a run leaves behind, as bytes"""
    d, (vk, n_in) = est.debug(), est.hypotheses()
    out = [bytes(est.result), d["valid"].tobytes(), d["rows"].tobytes(), d["samples"].tobytes(), bits(d["selected_abs_v"]).tobytes(), vk.tobytes(), n_in.tobytes()]
    for which in ("inliers", "outliers"):
        out += [a.tobytes() for a in est.to_numpy(which).values()]
    return out


@pytest.mark.gpu
def test_pcl_point_layout(mods):
    """the nodelet's points: 32-byte stride, intensity at float 4, doppler at float 5, padding that must not be read (NaN); host and device"""
    import torch
    _, ev, _ = mods
    tight = static_rows(300, 49)
    tight[[10, 200], 3] = F32(1.0)     # two rows fail the gate
    tight[[50, 51, 299], 4] += F32(5.0)  # three movers
    wide = np.full((300, 8), np.nan, dtype=F32)
    wide[:, :3], wide[:, 4], wide[:, 5] = tight[:, :3], tight[:, 3], tight[:, 4]
    cfg, words = E.Config(), words_for(3, 5, 4)
    est = ev.EgoVelocityEstimator(**params_of(cfg))
    ref, r = run_and_compare(ev, tight, cfg, words, est=est)
    assert ref.m == 298 and np.array_equal(ref.src[ref.outlier_rows], [50, 51, 299]) and not ref.merged
    want = snapshot(est)
    for cloud, cols in ((torch.from_numpy(tight).cuda(), (3, 4)), (wide, (4, 5)), (torch.from_numpy(wide).cuda(), (4, 5))):
        est.run(cloud, words=words, intensity_column=cols[0], doppler_column=cols[1])
        assert snapshot(est) == want


@pytest.mark.gpu
def test_one_handle_many_scans(mods, scene):
    """the way the class is used: one estimator, scan after scan of another n, m, K, S and mode; every run against the restatement, the first
    scan again at the end byte for byte what it was, and a refused call in between leaves the handle usable"""
    reg, ev, _ = mods
    big_cfg, small_cfg = E.Config(n_hypotheses=1024, N_ransac_points=8), E.Config(n_hypotheses=3, N_ransac_points=5)
    first = scan_with_m(scene, 4099, v_sensor=V_SENSOR, moving_share=0.02)
    w_big = words_for(1024, 8, 6)
    est = ev.EgoVelocityEstimator(**params_of(big_cfg))
    ref, r = run_and_compare(ev, first, big_cfg, w_big, est=est)
    assert ref.m == 4099 and ref.samples.shape == (1024, 8) and ref.success and not ref.zero_velocity and len(ref.outlier_rows) > 0
    want = snapshot(est)
    ref, r = run_and_compare(ev, scan_with_m(scene, 2, v_sensor=V_SENSOR, moving_share=0.0), big_cfg, w_big, est=est)
    assert ref.m == 2 and not ref.success and r.n_inlier == 0 and not est.hypotheses()[1].any() and not est.hypotheses()[0].any()
    ref, r = run_and_compare(ev, scene.raw_doppler_scan(2048, 21, (0.0, 0.0, 0.0), 0.02), big_cfg, w_big, est=est)
    assert ref.zero_velocity and r.best_in == -1 and not est.hypotheses()[1].any()
    with pytest.raises(reg.ApdgicpError) as e:
        est.run(first, words=w_big[:1023])   # too few words: refused before anything runs
    assert e.value.code == -1
    est.set_params(**params_of(small_cfg))
    ref, r = run_and_compare(ev, scan_with_m(scene, 65, v_sensor=V_SENSOR, moving_share=0.02), small_cfg, est=est)
    assert ref.m == 65 and ref.samples.shape == (3, 5) and ref.success and r.K == 3
    est.set_params(**params_of(big_cfg))
    run_and_compare(ev, first, big_cfg, w_big, est=est)
    assert snapshot(est) == want
