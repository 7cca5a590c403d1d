"""Every handle kind gives back what it allocated (riv-slam_amd/csrc/apd_devbuf.hpp: DevBuf / PinnedBuf free themselves, no owner lists its
buffers in a destructor).

apdgicp_debug_live_buffers counts the device and the pinned allocations the library's objects hold in the process.  One case per handle kind:
read the counts, create the object, run it on 64 points, run it again on 300 points (its buffers are replaced by larger ones), drop it, and
the counts are what they were -- not zero: fixtures of other modules may be alive.  The tests only count; the ownership mistakes themselves
(double free, use after free, a moved-from owner) are looked for on the CPU, tests/cpp/fake/test_devbuf.cpp under AddressSanitizer.
"""
import ctypes as C
import gc
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
F32 = np.float32
SIZES = (64, 300)


@pytest.fixture(scope="module")
def reg():
    import __graft_entry__ as g
    g.build()
    return importlib.import_module("riv-slam_amd.registration")


def mod(name):
    return importlib.import_module("riv-slam_amd." + name)


def live(reg):
    d, p = C.c_int64(-1), C.c_int64(-1)
    assert reg.load_library().apdgicp_debug_live_buffers(C.byref(d), C.byref(p)) == 0
    return d.value, p.value


def returns_what_it_took(reg, create, run, before_drop=None):
    gc.collect()
    start = live(reg)
    obj = create()
    for n in SIZES:
        run(obj, n)
    held = live(reg)
    assert held[0] > start[0], (start, held)   # (the object does hold counted buffers: the counter is wired to the allocations)
    if before_drop:
        before_drop(obj)
    del obj
    gc.collect()
    assert live(reg) == start, (start, held, live(reg))


def box_cloud(n, seed, columns=4):
    """n points in front of the sensor (x 2 .. 12 m, y +-5 m, z +-1 m), intensity 10"""
    rng = np.random.default_rng(seed)
    c = np.zeros((n, columns), dtype=F32)
    c[:, :3] = rng.uniform([2, -5, -1], [12, 5, 1], size=(n, 3))
    c[:, 3] = 10.0
    return c


def test_the_entry_point_takes_null_and_the_abi_version_stays(reg):
    L = reg.load_library()
    assert "apdgicp_debug_live_buffers" in reg.SYMBOLS and L.apdgicp_abi_version() == 6
    assert L.apdgicp_debug_live_buffers(None, None) == 0
    d, p = live(reg)
    assert d >= 0 and p >= 0


def test_registration_handle_plain_then_vgicp_then_ndt(reg, scene):
    vg, nd = mod("vgicp"), mod("ndt")
    vp, npar = vg.default_vgicp_params(), nd.default_ndt_params()
    vp.resolution = npar.resolution = 4.0

    def run(r, n):
        src, tgt, _, guess = scene.make_pair(n, n, scene.pair_seed(3, n), "odometry")
        r.setInputSource(src)
        r.setInputTarget(tgt)
        assert np.isfinite(r.align(guess)).all()
        reg._check(r.L.apdgicp_set_vgicp(r.h, C.byref(vp)))
        assert np.isfinite(r.align(guess)).all()
        reg._check(r.L.apdgicp_set_ndt(r.h, C.byref(npar)))      # (switches voxelized GICP off: the modes are exclusive)
        assert np.isfinite(r.align(guess)).all()
        r.swapSourceAndTarget()                                    # the maps go with their clouds
        reg._check(r.L.apdgicp_set_ndt(r.h, None))

    returns_what_it_took(reg, lambda: reg.FastAPDGICP(reg.default_params()), run)


def test_batch_handle_pooled_lm_then_vgicp_then_ndt_then_clear(reg, scene):
    vg, nd = mod("vgicp"), mod("ndt")
    vp, npar = vg.default_vgicp_params(), nd.default_ndt_params()
    vp.resolution = npar.resolution = 4.0

    def run(b, n):
        src, tgt, _, guess = scene.make_pair(n, n, scene.pair_seed(4, n), "odometry")
        b.set_clouds(0, [src, tgt])
        assert b.L.apdgicp_batch_is_pooled(b.b) > 0              # Levenberg-Marquardt: the pooled path
        assert np.isfinite(reg.result_matrix(b.align([(0, 1)], [guess])[0])).all()
        reg._check(b.L.apdgicp_batch_set_vgicp(b.b, C.byref(vp)))
        assert np.isfinite(reg.result_matrix(b.align([(0, 1)], [guess])[0])).all()
        reg._check(b.L.apdgicp_batch_set_ndt(b.b, C.byref(npar)))
        assert np.isfinite(reg.result_matrix(b.align([(0, 1)], [guess])[0])).all()
        reg._check(b.L.apdgicp_batch_set_ndt(b.b, None))

    def clear_gives_memory_back(b):
        held = live(reg)
        b.clear()
        assert live(reg)[0] < held[0], (held, live(reg))

    returns_what_it_took(reg, lambda: reg.BatchAPDGICP(reg.default_params(optimizer=reg.OPT_LM)), run, clear_gives_memory_back)


def test_submap_with_a_leaf(reg):
    def run(s, n):
        assert 0 < s.assemble([box_cloud(n, 1), box_cloud(n, 2)], leaf=0.5) <= 2 * n

    returns_what_it_took(reg, lambda: mod("submap").SubmapAssembler(), run)


def test_scan_filter_with_a_leaf_and_the_outlier_stage(reg):
    def run(f, n):
        assert 0 < f.run(box_cloud(n, 5)) <= n
        c = f.stage_counts()
        assert c[0] == n and c[2] > f.params.mean_k    # the outlier stage ran: the nested voxel grid and the nested engine exist

    returns_what_it_took(reg, lambda: mod("scan_filter").ScanFilter(leaf=0.1, outlier_method="STATISTICAL"), run)


def test_ego_velocity(reg):
    def run(e, n):
        c = box_cloud(n, 7, columns=5)
        d = c[:, :3] / np.linalg.norm(c[:, :3], axis=1, keepdims=True)
        c[:, 4] = -(d @ np.array([1.0, 0.2, 0.0], dtype=F32))
        res = e.run(c)
        assert res.m > 0 and res.n_inlier + res.n_outlier <= n

    returns_what_it_took(reg, lambda: mod("ego_velocity").EgoVelocityEstimator(), run)


def test_floor_detector_with_normal_filtering(reg):
    def run(f, n):
        rng = np.random.default_rng(n)
        c = np.zeros((n, 4), dtype=F32)
        c[:, :2] = rng.uniform(-10, 10, size=(n, 2))
        c[:, 2] = -2.0 + rng.normal(scale=0.02, size=n)    # the floor, sensor_height below the sensor
        res = f.run(c)
        assert res.n_clipped == n and n >= f.params.normal_k   # the normal filter searched: the nested engine exists

    returns_what_it_took(reg, lambda: mod("floor_detection").FloorDetector(use_normal_filtering=1), run)


def test_map_cloud_generator(reg):
    def run(m, n):
        kid = m.add_keyframe(box_cloud(n, 9))
        assert 0 < m.generate(np.stack([np.eye(4)] * (kid + 1)), resolution=0.1) <= sum(SIZES)

    def clear_gives_memory_back(m):
        held = live(reg)
        m.clear()
        assert live(reg)[0] < held[0], (held, live(reg))

    returns_what_it_took(reg, lambda: mod("map_cloud").MapCloudGenerator(), run, clear_gives_memory_back)


def test_scan_context_two_scans_one_query(reg):
    def run(s, n):
        a, b = s.add(box_cloud(n, 11)), s.add(box_cloud(n, 12))
        assert b == a + 1 and len(s.detect(b, [a], top_k=1).matches) <= 1

    returns_what_it_took(reg, lambda: mod("scan_context").ScanContext(), run)


def test_dbscan_two_blobs(reg):
    def run(h, n):
        rng = np.random.default_rng(n)
        blobs = np.concatenate([rng.normal(scale=0.1, size=(n // 2, 3)), rng.normal(scale=0.1, size=(n - n // 2, 3)) + [5, 0, 0]]).astype(F32)
        assert h.run(blobs) == 2

    returns_what_it_took(reg, lambda: mod("dbscan").DBSCAN(eps=1.0, min_pts=4), run)
