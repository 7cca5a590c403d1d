"""downsample_method APPROX_VOXELGRID without a GPU: the restatement of tests/approx_voxel_np.py on the cases include/apdgicp_hip.h works
out (AV1 .. AV7), its literal loop against its sort-and-scan form on every fixture the GPU tests use, and what the library and the Python
layer offer before a device is asked for anything."""
import ctypes as C
import importlib

import numpy as np
import pytest

import approx_voxel_np as A

F32 = np.float32
FIXTURE_NAMES = tuple(A.fixtures()) + ("big",)


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def test_worked_example_of_the_header():
    """leaf 1, order A, B, A', D: four points for three voxels -- A flushed by B, B by A', then A' and D from the final flush"""
    c = np.array([[0.5, 0.5, 0.5, 1], [512.5, 0.5, 0.5, 2], [0.25, 0.5, 0.5, 3], [1.5, 0.5, 0.5, 4]], dtype=F32)
    out, ijk, em = A.np_approx_voxel(c, 1.0)
    assert ijk.tolist() == [[0, 0, 0], [512, 0, 0], [0, 0, 0], [1, 0, 0]]
    assert A.voxel_hash(ijk).tolist() == [0, 0, 0, 3]
    assert np.array_equal(bits(out), bits(c)) and em.tolist() == [1, 2, -1, -1]
    assert np.array_equal(bits(A.np_approx_voxel_sorted(c, 1.0)), bits(c))


def test_hash_of_negative_indices_is_twos_complement():
    assert int(A.voxel_hash(np.array([-1, 0, 0]))) == 509
    assert int(A.voxel_hash(np.array([A.INT_MIN, 0, 0]))) == 0  # 2^31 * 7171 has no low 9 bits
    assert int(A.voxel_hash(np.array([-3, -7, 11]))) == ((-3 * 7171 - 7 * 3079 + 11 * 4231) & 511)


def test_an_index_an_int_cannot_hold_is_int_min_on_both_sides():
    c = np.array([[3e9, -3e9, 2147483648.0], [2147483520.0, -2147483648.0, 3e38], [0.5, -0.5, -0.0]], dtype=F32)
    assert A.voxel_indices(c, 1.0).tolist() == [[A.INT_MIN] * 3, [2147483520, A.INT_MIN, A.INT_MIN], [0, -1, 0]]
    assert A.voxel_indices(np.array([[3e38, 1, 1]], dtype=F32), 0.1)[0, 0] == A.INT_MIN  # an infinite product of finite factors


@pytest.mark.parametrize("name", FIXTURE_NAMES)
def test_literal_loop_equals_the_sort_and_scan_form(name):
    cloud, leaf, out, ijk, em = A.expected(name)
    part = A.takes_part(cloud)
    n_vox = len(np.unique(ijk[part], axis=0)) if part.any() else 0
    assert n_vox <= len(out) <= part.sum() and len(em) == len(out)
    assert np.array_equal(bits(out), bits(A.np_approx_voxel_sorted(cloud, leaf)))


def test_fixtures_hold_their_premises():
    n_vox = lambda name: len(np.unique(A.expected(name)[3][A.takes_part(A.expected(name)[0])], axis=0))
    assert len(A.expected("collisions")[2]) > n_vox("collisions") > 400           # re-emission (AV6)
    assert len(A.expected("alternation")[2]) == 600 and n_vox("alternation") == 2
    assert len(A.expected("sparse")[2]) == len(A.expected("sparse")[0]) == n_vox("sparse")
    a, b = A.expected("long_runs"), A.expected("long_runs_shuffled")
    assert len(a[2]) == len(b[2]) == 4 and A.LONG_RUN >= 2 * 1024
    assert np.array_equal(np.unique(a[3], axis=0), np.unique(b[3], axis=0)) and a[2].tobytes() != b[2].tobytes()
    assert (A.expected("overflow")[3] == A.INT_MIN).sum() == 5 and (A.expected("negative")[3] < 0).all()
    cloud, bad = A.holes_cloud()
    assert not A.takes_part(cloud)[bad].any() and A.takes_part(cloud).sum() == len(cloud) - len(bad)
    # a hole changes nothing for the others: the cloud without its holes gives the same bytes
    assert A.np_approx_voxel(cloud[A.takes_part(cloud)], 0.5)[0].tobytes() == A.expected("holes")[2].tobytes()
    assert A.BIG_N > 2 ** 17 and len(A.expected("big")[0]) == A.BIG_N


def test_params_carry_the_method_and_keep_their_size():
    sf = importlib.import_module("riv-slam_amd.scan_filter")
    assert C.sizeof(sf.ScanFilterParams) == 80 and sf.ScanFilterParams.downsample_method.offset == 76
    assert sf.default_filter_params().downsample_method == 0
    assert sf.default_filter_params(downsample_method="APPROX_VOXELGRID").downsample_method == 1
    assert sf.default_filter_params(downsample_method="VOXELGRID").downsample_method == 0
    assert sf.default_filter_params(downsample_method=1).downsample_method == 1
    with pytest.raises(KeyError):
        sf.default_filter_params(downsample_method="OCTREE")


def test_library_exports_the_setter_and_checks_its_arguments_first():
    reg = importlib.import_module("riv-slam_amd.registration")
    L = reg.load_library()
    assert "apdgicp_submap_set_downsample_method" in reg.SYMBOLS and hasattr(L, "apdgicp_submap_set_downsample_method")
    assert L.apdgicp_submap_set_downsample_method(None, 1) == -1  # APDGICP_ERR_INVALID_ARG
    assert L.apdgicp_submap_set_downsample_method(None, 0) == -1
    assert L.apdgicp_abi_version() == 6
