"""The covariance k-NN (k_knn_cov_coop, riv-slam_amd/csrc/apd_kernels.hpp) keeps what a step of phase B needs of its query -- q, tau, the
list count -- in a per-query record in LDS and reads it from a wave-uniform address, where it used to broadcast registers with v_readlane.
That is data movement only: every covariance must be, bit for bit, what the brute-force kernel (APDGICP_KNN_MODE=brute) computes.

What can go wrong is ordering, and each shape below is the smallest that reaches one of the hazards:
  n = 20 (= k), 21, 65       one partial wave, clouds smaller than the 128-point window, a last wave with ONE valid query: padding queries
                             carry tau = -1 in their record and must get no group;
  n = 129, 257, thin strip   every query near a group edge needs two or three consecutive groups: the same query closes one group and opens
                             the next, its record is read again right behind the write of its count (and of a tightened tau);
  n = 200, 100 in a 1 cm blob  more than 60 hits in a query's first group: a tightening rewrites tau in the record in the query's first step,
                             and the step in the next group must see it;
  6 x 6 x 6 lattice          exact fp32 distance ties by the hundred: the low word of tau (the index) decides membership;
  one 8 192-point cloud of the benchmark (scene.pair_seed(2, 0)).

The instantiation depends on the points of the launch (apd_engine.hpp, launch_knn): 16 lanes per query below 40 000, 8 below 100 000, 4 (sixteen
queries per wave, the benchmark's) from there.  So every cloud is run alone (i), with five (ii) and with thirteen (iii) 8 192-point filler clouds
in the same launch.

The observable is the batch handle's voxel map of the cloud (apdgicp_batch_vgicp_get_voxels) at a resolution of 1 mm: the sum of the point
covariances of each voxel, nearly everywhere one point per voxel.  A covariance is the fp64 moment sum over the k neighbours in rank order, so
a wrong neighbour, a missing one or another order changes its bits: the neighbour lists are checked through it.  The reference map comes from
a second handle created under APDGICP_KNN_MODE=brute, once per shape, holding the cloud alone (the brute-force kernel has one instantiation)."""
import importlib

import numpy as np
import pytest

gpu = pytest.mark.gpu
RES = 1e-3
FILLERS = {"alone_16_lanes": 0, "fillers_8_lanes": 5, "fillers_4_lanes": 13}
LAUNCH_TOTAL = {"alone_16_lanes": (0, 40000), "fillers_8_lanes": (40000, 100000), "fillers_4_lanes": (100000, 1 << 30)}


def _strip(n):
    """n points along x, 5 cm apart, 1 mm of jitter across: a 128-point group of the sorted cloud is a few segments of the strip, and a
    query near a segment's end has its 20 neighbours in two or three groups"""
    rng = np.random.default_rng(n)
    p = np.zeros((n, 3))
    p[:, 0] = 0.05 * np.arange(n) + rng.uniform(-0.01, 0.01, n)
    p[:, 1:] = rng.uniform(-1e-3, 1e-3, (n, 2))
    return p[rng.permutation(n)].astype(np.float32)


def _blob():
    rng = np.random.default_rng(200)
    return np.concatenate([rng.uniform(-0.005, 0.005, (100, 3)) + [3.0, 1.0, 0.5], rng.uniform(-4, 4, (100, 3)) * [1, 1, 0.2]]).astype(np.float32)


def _lattice():
    g = np.arange(6, dtype=np.float32) * np.float32(0.25)   # exactly representable: equal distances are equal floats
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)[np.random.default_rng(6).permutation(216)]


def _uniform(n):
    return (np.random.default_rng(n).normal(size=(n, 3)) * [5, 5, 1]).astype(np.float32)


SHAPES = {
    "n20": lambda scene: _uniform(20),
    "n21": lambda scene: _uniform(21),
    "n65": lambda scene: _uniform(65),
    "strip129": lambda scene: _strip(129),
    "strip257": lambda scene: _strip(257),
    "blob200": lambda scene: _blob(),
    "lattice216": lambda scene: _lattice(),
    "bench8192": lambda scene: scene.make_pair(8192, 8192, scene.pair_seed(2, 0))[0],
}


@pytest.fixture(scope="module")
def reg():
    import __graft_entry__ as g
    g.build()
    return importlib.import_module("riv-slam_amd.registration")


@pytest.fixture(scope="module")
def vg(reg):
    return importlib.import_module("riv-slam_amd.vgicp")


@pytest.fixture(scope="module")
def fillers(scene):
    """thirteen 8 192-point scene clouds, on the device once"""
    import torch
    out = []
    for p in range(7):
        s, t, _, _ = scene.make_pair(8192, 8192, scene.pair_seed(2, 1 + p))
        out += [torch.from_numpy(np.ascontiguousarray(s)).cuda(), torch.from_numpy(np.ascontiguousarray(t)).cuda()]
    return out[:13]


def _voxel_map(reg, vg, monkeypatch, mode, clouds):
    """the voxel map of clouds[0] after ONE covariance launch over all of `clouds`, from a handle created under the given k-NN mode"""
    if mode == "brute":
        monkeypatch.setenv("APDGICP_KNN_MODE", "brute")   # (read when the handle's engine is created)
    else:
        monkeypatch.delenv("APDGICP_KNN_MODE", raising=False)
    b = vg.BatchVGICP(reg.default_params())
    try:
        b.setResolution(RES)
        b.set_clouds(0, clouds)
        b.compute_covariances()
        return b.voxels(0)
    finally:
        b.close()


_reference = {}


def _brute(reg, vg, scene, monkeypatch, shape):
    """computed once per shape, shared by the three variants, never written to"""
    if shape not in _reference:
        import torch
        cloud = SHAPES[shape](scene)
        m = _voxel_map(reg, vg, monkeypatch, "brute", [torch.from_numpy(np.ascontiguousarray(cloud)).cuda()])
        for a in m.values():
            a.setflags(write=False)
        _reference[shape] = (cloud, m)
    return _reference[shape]


def test_the_shapes_are_what_the_cases_need(scene):
    """(no device) sizes, the launch totals of the three variants, the blob and the lattice's exact ties"""
    sizes = {k: len(f(scene)) for k, f in SHAPES.items()}
    assert sizes == {"n20": 20, "n21": 21, "n65": 65, "strip129": 129, "strip257": 257, "blob200": 200, "lattice216": 216, "bench8192": 8192}
    for variant, nf in FILLERS.items():
        lo, hi = LAUNCH_TOTAL[variant]
        for n in sizes.values():
            assert lo <= n + 8192 * nf < hi, (variant, n)
    b = _blob().astype(np.float64)
    assert (np.abs(b[:100] - [3.0, 1.0, 0.5]).max(axis=1) <= 0.005 + 1e-6).all()   # 100 points inside a 1 cm cube: > 60 within any tau
    lat = _lattice()
    d = ((lat[:, None, :] - lat[None, :, :]) ** 2).sum(-1, dtype=np.float32)
    assert (d == np.float32(0.0625)).sum() == 2 * 3 * 5 * 36   # every lattice edge, both ways: the same float
    s = np.sort(_strip(257)[:, 0])
    assert np.all(np.diff(s) > 0.02) and s[-1] - s[0] > 12.0   # a strip: 257 distinct places along x, 1 mm wide


@gpu
@pytest.mark.parametrize("variant", list(FILLERS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_covariances_are_bitwise_the_brute_force_kernels(reg, vg, scene, fillers, monkeypatch, shape, variant):
    import torch
    cloud, want = _brute(reg, vg, scene, monkeypatch, shape)
    got = _voxel_map(reg, vg, monkeypatch, "pruned", [torch.from_numpy(np.ascontiguousarray(cloud)).cuda()] + fillers[:FILLERS[variant]])
    assert len(want["counts"]) > 0 and int(want["counts"].sum()) == len(cloud)
    assert np.array_equal(got["coords"], want["coords"]) and np.array_equal(got["counts"], want["counts"])
    assert np.array_equal(got["means"].view(np.uint64), want["means"].view(np.uint64))
    bad = np.flatnonzero((got["covs"].view(np.uint64) != want["covs"].view(np.uint64)).reshape(len(want["counts"]), -1).any(axis=1))
    assert bad.size == 0, f"{bad.size} of {len(want['counts'])} voxels differ from the brute-force kernel's, first at {want['coords'][bad[0]]}"
