"""downsample_method APPROX_VOXELGRID on the device (riv-slam_amd/csrc/apd_approx_voxel.hpp; include/apdgicp_hip.h, AV1 .. AV7), through
SubmapAssembler and through ScanFilter with the gate off and no outlier filter.

The bar everywhere: the device output equals the bytes of the literal loop of tests/approx_voxel_np.py -- n_out, every float, the order.
The algorithm has no tolerance to give: every fp32 operation and its order are stated.  Each fixture's premise is asserted on the
restatement alone before the device is asked (and, without a GPU, in tests/test_approx_voxel_cpu.py).  The outlier filters behind the new
step-2 cloud keep the bars of tests/test_scan_filter.py (scores bit for bit; mean / stddev / thr within 1e-9 relative, the rounding of a
fixed-tree against a sequential sum of fewer than 2^17 doubles; the mask identical once no score lies within 1e-9 thr of thr)."""
import importlib

import numpy as np
import pytest

import approx_voxel_np as A
from scan_filter_np import knn_d2_kdtree, np_radius, np_range_gate, np_statistical

F32 = np.float32
pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


@pytest.fixture(scope="module")
def mods():
    import __graft_entry__ as g
    g.build()
    return (importlib.import_module("riv-slam_amd.registration"), importlib.import_module("riv-slam_amd.scan_filter"),
            importlib.import_module("riv-slam_amd.submap"))


@pytest.fixture(scope="module")
def assembler(mods):
    return mods[2].SubmapAssembler()


@pytest.fixture(scope="module")
def scan_filter(mods):
    return mods[1].ScanFilter(use_distance_filter=0, outlier_method="NONE", downsample_method="APPROX_VOXELGRID")


def assert_both_paths(assembler, scan_filter, cloud, leaf, want):
    n = assembler.assemble([cloud], None, leaf, method="APPROX_VOXELGRID")
    got = assembler.to_numpy()
    assert n == len(want) and np.array_equal(bits(got), bits(want))
    scan_filter.set_params(leaf=leaf)
    n = scan_filter.run(cloud)
    assert n == len(want) and np.array_equal(bits(scan_filter.to_numpy()), bits(want))
    assert scan_filter.stage_counts() == (len(cloud), len(cloud), n, n)


@pytest.mark.parametrize("name", [f"n{n}" for n in A.SIZES] + ["big"])
def test_sizes_around_every_block(assembler, scan_filter, name):
    """0, 1, 2, one below / at / one above the 64-lane wave, AV_BLK = 256, SCAN_BLK = 1024 and the 4096 keys of a scan tile and a radix
    tile, two tiles and a bit, and 2^17 + 1 points (513 blocks of 256, 33 tiles)"""
    cloud, leaf, want, ijk, _ = A.expected(name)
    assert_both_paths(assembler, scan_filter, cloud, leaf, want)


def test_collisions_emit_a_voxel_more_than_once(assembler, scan_filter):
    cloud, leaf, want, ijk, em = A.expected("collisions")
    n_vox = len(np.unique(ijk, axis=0))
    assert len(want) > n_vox and (em >= 0).sum() == len(want) - len(np.unique(A.voxel_hash(ijk)))
    assert_both_paths(assembler, scan_filter, cloud, leaf, want)
    # ... and not in ascending voxel order, which is what the exact grid returns for the same cloud
    assert assembler.assemble([cloud], None, leaf, method="VOXELGRID") == n_vox


def test_alternation_emits_every_point(assembler, scan_filter):
    cloud, leaf, want, ijk, em = A.expected("alternation")
    assert len(want) == len(cloud) == 600 and len(np.unique(ijk, axis=0)) == 2 and (A.voxel_hash(ijk) == 0).all()
    assert np.array_equal(bits(want), bits(cloud))   # every run is one point, flushed by the next
    assert_both_paths(assembler, scan_filter, cloud, leaf, want)


def test_long_runs_keep_input_order_across_block_edges(assembler, scan_filter):
    a, b = A.expected("long_runs"), A.expected("long_runs_shuffled")
    assert len(a[2]) == len(b[2]) == 4 and A.LONG_RUN >= 2 * 1024
    assert np.array_equal(np.unique(a[3], axis=0), np.unique(b[3], axis=0)) and a[2].tobytes() != b[2].tobytes()
    assert_both_paths(assembler, scan_filter, a[0], a[1], a[2])
    assert_both_paths(assembler, scan_filter, b[0], b[1], b[2])


def test_sparse_cloud_comes_back_reordered(assembler, scan_filter):
    cloud, leaf, want, ijk, em = A.expected("sparse")
    assert len(want) == len(cloud) == len(np.unique(ijk, axis=0))
    assert sorted(map(bytes, want)) == sorted(map(bytes, cloud)) and want.tobytes() != cloud.tobytes()
    assert_both_paths(assembler, scan_filter, cloud, leaf, want)


@pytest.mark.parametrize("name", ("negative", "faces", "anisotropic", "overflow", "holes"))
def test_index_edges(assembler, scan_filter, name):
    cloud, leaf, want, ijk, _ = A.expected(name)
    part = A.takes_part(cloud)
    if name == "negative":
        assert (ijk < 0).all()
    elif name == "faces":
        on_face = (cloud[:, :3] / F32(0.25) == np.round(cloud[:, :3] / F32(0.25))).all(1)
        assert on_face.sum() >= 1000 and (cloud[:, :3] < 0).any()
    elif name == "anisotropic":
        assert len(set(np.broadcast_to(leaf, (3,)).tolist())) == 3
    elif name == "overflow":
        assert (ijk == A.INT_MIN).sum() == 5 and (cloud[:, :3][ijk == A.INT_MIN] > 0).sum() == 4 and part.all()
    else:
        assert (~part).sum() == 62 and not part[0] and not part[-1]
        assert A.np_approx_voxel(cloud[part], leaf)[0].tobytes() == want.tobytes()  # the others are where they would be without the holes
    assert_both_paths(assembler, scan_filter, cloud, leaf, want)


def test_intensity_present_absent_or_elsewhere(assembler):
    cloud, leaf, want, _, _ = A.expected("collisions")
    zero = np.ascontiguousarray(np.concatenate([cloud[:, :3], np.zeros((len(cloud), 1), dtype=F32)], 1))
    want0 = A.np_approx_voxel(zero, leaf)[0]
    assert not want0[:, 3].any() and np.array_equal(bits(want0[:, :3]), bits(want[:, :3]))
    assert assembler.assemble([cloud], None, leaf, intensity_column=None, method="APPROX_VOXELGRID") == len(want0)
    assert np.array_equal(bits(assembler.to_numpy()), bits(want0))
    assert assembler.assemble([np.ascontiguousarray(cloud[:, :3])], None, leaf, method=1) == len(want0)  # a column the cloud does not have
    assert np.array_equal(bits(assembler.to_numpy()), bits(want0))
    wide = np.zeros((len(cloud), 8), dtype=F32)   # pcl::PointXYZI: 32-byte points, intensity at byte 16
    wide[:, :3], wide[:, 3], wide[:, 4] = cloud[:, :3], 7.0, cloud[:, 3]
    assert assembler.assemble([wide], None, leaf, intensity_column=4, method="APPROX_VOXELGRID") == len(want)
    assert np.array_equal(bits(assembler.to_numpy()), bits(want))


def test_host_and_device_input_give_the_same_bytes(mods, assembler, scan_filter):
    import torch
    cloud, leaf, want, _, _ = A.expected("n4097")
    dev = torch.from_numpy(np.array(cloud)).cuda()
    assert assembler.assemble([dev], None, leaf, method="APPROX_VOXELGRID") == len(want)
    assert np.array_equal(bits(assembler.to_numpy()), bits(want))
    scan_filter.set_params(leaf=leaf)
    assert scan_filter.run(dev) == len(want) and np.array_equal(bits(scan_filter.to_numpy()), bits(want))
    pts = mods[2].approx_voxel_downsample(dev, leaf)   # the align.cpp / kitti.cpp protocol: one cloud, no poses
    assert pts.n == len(want)
    back = np.empty((pts.n, 4), dtype=F32)
    mods[0]._check(mods[0].load_library().apdgicp_submap_copy(pts.owner.h, mods[0]._ptr(back), pts.n, 0))
    assert np.array_equal(bits(back), bits(want))


def test_reuse_of_one_handle(mods):
    sub = mods[2]
    a = sub.SubmapAssembler()
    cloud, leaf, want, ijk, _ = A.expected("collisions")
    small = A.expected("n65")
    big = A.expected("n8193")
    assert a.assemble([cloud], None, leaf, method="APPROX_VOXELGRID") == len(want)
    first = a.to_numpy()
    n_exact = a.assemble([cloud], None, leaf, method="VOXELGRID")
    exact = a.to_numpy()
    fresh = sub.SubmapAssembler()
    assert fresh.assemble([cloud], None, leaf) == n_exact == len(np.unique(ijk, axis=0)) and exact.tobytes() == fresh.to_numpy().tobytes()
    assert a.assemble([cloud], None, leaf, method="APPROX_VOXELGRID") == len(want)
    assert first.tobytes() == a.to_numpy().tobytes() == want.tobytes()
    # a large cloud, then a small one: nothing of the large one's runs is left in the buffers
    assert a.assemble([big[0]], None, big[1], method="APPROX_VOXELGRID") == len(big[2]) and a.to_numpy().tobytes() == big[2].tobytes()
    assert a.assemble([small[0]], None, small[1], method="APPROX_VOXELGRID") == len(small[2]) and a.to_numpy().tobytes() == small[2].tobytes()
    assert a.assemble([small[0]], None, small[1], method="APPROX_VOXELGRID") == len(small[2]) and a.to_numpy().tobytes() == small[2].tobytes()
    # the method stays on the object (the C ABI's setter is sticky; assemble()'s keyword sets it every time)
    L = mods[0].load_library()
    assert L.apdgicp_submap_set_downsample_method(a.h, 2) == -1 and L.apdgicp_submap_set_downsample_method(a.h, -1) == -1


def test_submap_of_three_clouds_with_poses(mods, scene):
    sub = mods[2]
    rng = np.random.default_rng(17)
    clouds = [np.ascontiguousarray(np.concatenate([rng.uniform(-6, 6, (m, 3)), rng.uniform(0, 40, (m, 1))], 1).astype(F32)) for m in (1500, 700, 1101)]
    poses = [scene.make_transform([0.4 * i, -0.2 * i, 0.1], 0.03 * i, -0.01, 0.02 * i).astype(np.float64) for i in range(3)]
    a = sub.SubmapAssembler()
    assert a.assemble(clouds, poses, None, method="APPROX_VOXELGRID") == 3301
    cat = a.to_numpy()   # the transformed concatenation (leaf None: NONE, whatever the method)
    want, ijk, _ = A.np_approx_voxel(cat, 0.4)
    assert len(np.unique(ijk, axis=0)) < len(want) < len(cat)
    assert a.assemble(clouds, poses, 0.4, method="APPROX_VOXELGRID") == len(want)
    assert np.array_equal(bits(a.to_numpy()), bits(want))
    pts = a.points()
    assert pts.n == len(want)


def test_whole_filter_gate_approx_grid_and_outlier_filters(mods, scene):
    sf = mods[1]
    c = scene.raw_scan(2048, 2)
    keep = np_range_gate(c)
    s2, ijk, _ = A.np_approx_voxel(c[keep], 0.1)
    assert 0 < keep.sum() < len(c) and 100 < len(s2) <= keep.sum()
    f = sf.ScanFilter(outlier_method="NONE", downsample_method="APPROX_VOXELGRID")
    assert f.run(c) == len(s2) and np.array_equal(bits(f.to_numpy()), bits(s2))
    assert f.stage_counts() == (len(c), keep.sum(), len(s2), len(s2))
    mean_k, mul = 20, 1.0
    score, mean, stddev, thr, kept = np_statistical(knn_d2_kdtree(s2, mean_k + 1), mean_k, mul)
    assert np.abs(score.astype(np.float64) - thr).min() > 1e-9 * thr and 0 < kept.sum() < len(s2)   # conditions on the input
    f.set_params(outlier_method="STATISTICAL", mean_k=mean_k, stddev_mul=mul)
    n = f.run(c)
    sc = f.scores()
    rel = max(abs(sc["mean"] - mean) / mean, abs(sc["stddev"] - stddev) / stddev, abs(sc["thr"] - thr) / thr)
    print(f"STATISTICAL: n2 {len(s2)} kept {kept.sum()} sums rel diff {rel:.2e}")
    assert np.array_equal(bits(sc["stat"]), bits(score)) and rel <= 1e-9
    assert np.array_equal(sc["kept"], kept) and n == kept.sum() and np.array_equal(bits(f.to_numpy()), bits(s2[kept]))
    assert f.stage_counts() == (len(c), keep.sum(), len(s2), n)
    radius, mn = 0.8, 2
    stat, kept = np_radius(knn_d2_kdtree(s2, mn + 1), mn, radius)
    assert not (stat.astype(np.float64) == radius * radius).any() and 0 < kept.sum() < len(s2)
    f.set_params(outlier_method="RADIUS", radius=radius, min_neighbors=mn)
    n = f.run(c)
    sc = f.scores()
    assert np.array_equal(bits(sc["stat"]), bits(stat)) and sc["thr"] == radius * radius
    assert np.array_equal(sc["kept"], kept) and n == kept.sum() and np.array_equal(bits(f.to_numpy()), bits(s2[kept]))
    assert f.stage_counts() == (len(c), keep.sum(), len(s2), n)


def test_parameter_checks(mods, scan_filter):
    reg, sf, sub = mods
    assert reg.load_library().apdgicp_abi_version() == 6
    p = sf.default_filter_params(downsample_method=2)
    with pytest.raises(reg.ApdgicpError) as e:
        sf.ScanFilter(p)
    assert e.value.code == -1
    with pytest.raises(reg.ApdgicpError) as e:
        scan_filter.set_params(downsample_method=2)
    assert e.value.code == -1 and scan_filter.params.downsample_method == 1   # (the handle keeps what it had)
    cloud = A.expected("n257")[0]
    f = sf.ScanFilter(use_distance_filter=0, outlier_method="NONE", leaf=None, downsample_method="APPROX_VOXELGRID")
    assert f.run(cloud) == len(cloud) and np.array_equal(bits(f.to_numpy()), bits(cloud))   # leaf None: NONE, whatever the method
    a = sub.SubmapAssembler()
    assert a.assemble([cloud], None, None, method="APPROX_VOXELGRID") == len(cloud) and np.array_equal(bits(a.to_numpy()), bits(cloud))
    with pytest.raises(reg.ApdgicpError) as e:
        a.assemble([cloud], None, 0.5, method=7)
    assert e.value.code == -1
