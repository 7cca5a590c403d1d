"""FAST_VGICP_CUDA as a mode of the registration handle, the part that needs no GPU: exports, defaults, the offset lists of VC6 from the
library against the restatement (tests/vgicp_cuda_np.py), the parameter checks that need no handle, and self-checks of the restatement
and of the fixture (tests/golden/vgicp_cuda_pair.npz, made by tests/golden/make_vgicp_cuda_golden.py)."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest

import vgicp_cuda_np as VC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("apdgicp_vgicp_cuda_default_params", "apdgicp_set_vgicp_cuda", "apdgicp_get_vgicp_cuda", "apdgicp_vgicp_cuda_offsets", "apdgicp_vgicp_cuda_kept",
               "apdgicp_vgicp_cuda_get_covariances", "apdgicp_vgicp_cuda_voxel_count", "apdgicp_vgicp_cuda_get_voxels", "apdgicp_vgicp_cuda_get_correspondences",
               "apdgicp_vgicp_cuda_build_count")
RADIUS_COUNTS = {0.0: 1, 0.5: 1, 1.0: 7, 1.5: 19, 2.0: 33, 2.5: 81, 3.0: 123, 4.0: 257}   # VC6
SIZES = (20, 21, 63, 64, 65, 255, 256, 257, 2048)


@pytest.fixture(scope="module")
def reg():
    import __graft_entry__ as g
    g.build()
    return importlib.import_module("riv-slam_amd.registration")


@pytest.fixture(scope="module")
def vc(reg):
    return importlib.import_module("riv-slam_amd.vgicp_cuda")


@pytest.fixture(scope="module")
def pair():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "vgicp_cuda_pair.npz")))


def test_new_symbols_are_exported_and_the_module_imports(reg, vc):
    L = reg.load_library()
    header = open(os.path.join(ROOT, "include", "apdgicp_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), f"{name} is not exported"
        assert name in reg.SYMBOLS
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared"
    for m in ("setResolution", "setKernelWidth", "setRegularizationMethod", "setNeighborSearchMethod", "setNearestNeighborSearchMethod", "setCorrespondenceRandomness",
              "swapSourceAndTarget", "clearSource", "clearTarget", "setInputSource", "setInputTarget", "align", "kept", "covariances", "voxels", "voxel_correspondences"):
        assert callable(getattr(vc.FastVGICPCuda, m))
    assert issubclass(vc.FastVGICPCuda, reg.FastAPDGICP)
    assert L.apdgicp_abi_version() == 6
    for k in range(1, 11):
        assert f"VC{k}." in header


def test_default_params(vc):
    p = vc.default_vgicp_cuda_params()
    assert (p.resolution, p.neighbor_search, p.search_radius, p.regularization, p.nn_method) == (1.0, vc.DIRECT1, 1.5, vc.PLANE, vc.CPU_PARALLEL_KDTREE)
    assert ctypes.sizeof(vc.VgicpCudaParams) == 32
    assert (VC.DIRECT1, VC.DIRECT7, VC.DIRECT27, VC.DIRECT_RADIUS) == (vc.DIRECT1, vc.DIRECT7, vc.DIRECT27, vc.DIRECT_RADIUS)
    assert (VC.MIN_EIG, VC.PLANE, VC.FROBENIUS) == (vc.MIN_EIG, vc.PLANE, vc.FROBENIUS)


def _params(vc, **kw):
    p = vc.default_vgicp_cuda_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_offset_counts_and_order(vc):
    for r, count in RADIUS_COUNTS.items():
        got = vc.neighbor_offsets(_params(vc, neighbor_search=vc.DIRECT_RADIUS, search_radius=r))
        want = VC.neighbor_offsets(VC.DIRECT_RADIUS, r)
        assert len(got) == count and np.array_equal(got, want), r
        assert np.abs(got).max() <= 4
    # the order: i slowest, k fastest
    assert VC.neighbor_offsets(VC.DIRECT_RADIUS, 1.0).tolist() == [[-1, 0, 0], [0, -1, 0], [0, 0, -1], [0, 0, 0], [0, 0, 1], [0, 1, 0], [1, 0, 0]]
    o15 = VC.neighbor_offsets(VC.DIRECT_RADIUS, 1.5).tolist()
    assert o15 == [[i, j, k] for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1) if abs(i) + abs(j) + abs(k) <= 2]
    assert o15[0] == [-1, -1, 0] and o15[9] == [0, 0, 0] and o15[-1] == [1, 1, 0]
    # sqrt(2) = 1.41421...: 1.41 + 1e-3 is below it, 1.42 above
    assert len(vc.neighbor_offsets(_params(vc, neighbor_search=vc.DIRECT_RADIUS, search_radius=1.41))) == 7
    assert len(vc.neighbor_offsets(_params(vc, neighbor_search=vc.DIRECT_RADIUS, search_radius=1.42))) == 19
    for m in (vc.DIRECT1, vc.DIRECT7, vc.DIRECT27):
        assert np.array_equal(vc.neighbor_offsets(_params(vc, neighbor_search=m)), VC.neighbor_offsets(m))
    # the radius is not read without DIRECT_RADIUS
    assert len(vc.neighbor_offsets(_params(vc, neighbor_search=vc.DIRECT7, search_radius=float("nan")))) == 7


@pytest.mark.parametrize("kw, code", [
    (dict(nn_method=2), -5),                                  # GPU_RBF_KERNEL
    (dict(regularization=0), -5),                             # NONE
    (dict(regularization=2), -5),                             # NORMALIZED_MIN_EIG
    (dict(neighbor_search=3, search_radius=-0.5), -1),
    (dict(neighbor_search=3, search_radius=4.5), -1),
    (dict(neighbor_search=3, search_radius=float("nan")), -1),
    (dict(neighbor_search=3, search_radius=float("inf")), -1),
    (dict(resolution=0.0), -1),
    (dict(resolution=-1.0), -1),
    (dict(resolution=float("nan")), -1),
    (dict(neighbor_search=4), -1),
    (dict(regularization=7), -1),
    (dict(nn_method=3), -1),
])
def test_parameter_checks_that_need_no_handle(reg, vc, kw, code):
    with pytest.raises(reg.ApdgicpError) as ei:
        vc.neighbor_offsets(_params(vc, **kw))
    assert ei.value.code == code, str(ei.value)


def _brute_knn(cloud, k):
    """every pair, fp32, (distance, index) order: written without the oracle's k-NN"""
    c = cloud.astype(np.float32)
    out = np.empty((len(c), k), dtype=np.int64)
    for i in range(len(c)):
        d = c - c[i]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        out[i] = np.lexsort((np.arange(len(c)), d2))[:k]
    return out


def test_restatement_filter_against_a_brute_force_knn(pair):
    for name in ("source", "target"):
        cloud = pair[name]
        nb = _brute_knn(cloud, VC.K)
        p = VC.prepare(cloud)
        assert np.array_equal(p["neighbours"], nb)
        assert (nb[:, 0] == np.arange(len(cloud))).all()      # the point itself first
        # the raw covariance of VC2 is the population covariance of the 20 neighbours
        want = np.array([np.cov(cloud[nb[i]].astype(np.float64).T, bias=True) for i in range(len(cloud))])
        assert np.abs(p["raw_all"] - want).max() <= 1e-9 * max(1.0, np.abs(cloud).max() ** 2)
        w = np.linalg.eigvalsh(want)
        keep = w[:, 1] > 0.1 * w[:, 2]
        assert np.array_equal(np.nonzero(keep)[0], p["kept_index"]) and np.array_equal(p["kept_index"], pair[f"{name}_kept"])
        # a kept point's covariance: eigenvalues (1e-3, 1, 1), the 1e-3 along the raw covariance's smallest direction
        wr, Ur = np.linalg.eigh(p["covs"])
        assert np.abs(wr - [1e-3, 1.0, 1.0]).max() <= 1e-12
        _, U = np.linalg.eigh(p["raw"])
        assert np.abs(np.abs(np.einsum("ni,ni->n", Ur[:, :, 0], U[:, :, 0])) - 1.0).max() <= 1e-9


def test_restatement_raw_covariance_is_the_literal_loop(pair):
    cloud = pair["target"][:257]
    nb = VC.neighbours(cloud)
    got = VC.raw_covariances(cloud, nb)
    P = cloud.astype(np.float64)
    for i in (0, 1, 100, 256):
        mean, cov = np.zeros(3), np.zeros((3, 3))
        for r in range(VC.K):                                  # CE:26-34, line for line
            pt = P[nb[i, r]]
            mean = mean + pt
            cov = cov + np.outer(pt, pt)
        mean = mean / VC.K
        cov = cov / VC.K - np.outer(mean, mean)
        assert np.array_equal(cov.view(np.uint64), got[i].view(np.uint64))


def test_fixture_meets_its_conditions(pair):
    for name in ("source", "target"):
        for n in SIZES:
            c = VC.filter_conditions(VC.raw_covariances(pair[name][:n], VC.neighbours(pair[name][:n])))
            assert c["threshold_margin"] > 1e-9 and c["gap_margin"] >= 1e-6, (name, n, c)
        assert 0.05 <= c["dropped"] <= 0.50, (name, c)
    # the edge cases of the size list: the 20-point prefixes are kept whole, the line cloud is dropped whole
    assert len(VC.prepare(pair["source"][:20])["kept_index"]) == 20 and len(VC.prepare(pair["target"][:20])["kept_index"]) == 20
    assert len(VC.prepare(pair["line"])["kept_index"]) == 0
    assert np.linalg.norm(np.diff(pair["line"], axis=0), axis=1).min() > 0     # noise, not a degenerate copy


def test_restatement_regularisations_without_a_filter(pair):
    cloud = pair["source"][:300]
    raw = VC.raw_covariances(cloud, VC.neighbours(cloud))
    keep, c = VC.regularize(raw, VC.MIN_EIG)
    assert keep.all() and np.linalg.eigvalsh(c).min() >= 1e-3 * (1 - 1e-9)
    big = np.linalg.eigvalsh(raw).min(axis=1) >= 1e-3
    assert big.any() and np.abs(c[big] - raw[big]).max() <= 1e-12 * np.abs(raw).max()
    keep, c = VC.regularize(raw, VC.FROBENIUS)
    assert keep.all()
    Ci = np.linalg.inv(raw + 1e-3 * np.eye(3))
    want = (raw + 1e-3 * np.eye(3)) * np.sqrt((Ci * Ci).sum(axis=(1, 2)))[:, None, None]
    assert np.abs(c - want).max() <= 1e-9 * np.abs(want).max()
    with pytest.raises(NotImplementedError):
        VC.regularize(raw, 0)
