"""numpy restatement of the scan filter (riv-slam_amd/csrc/apd_filter.hpp) in the operation orders include/apdgicp_hip.h states (section
"scan preprocessing"; PCL as published): the expected values of tests/test_scan_filter.py.  The k-NN distances come from the checker's
kd-tree (ref.RefAPDGICP.knn_kdtree_batch, pinned bit for bit to the reference tree's nanoflann by tests/test_oracle.py) or from a chunked
numpy brute force in FLANN L2_Simple order.  Every fp32 operation is a numpy float32 operation."""
import numpy as np

import ref as R

F32 = np.float32


def np_range_gate(cloud, near=1.0, far=100.0, z_low=-5.0, z_high=20.0):
    """preprocessing_nodelet.cpp:881-889: d = fp32 sqrtf((x*x + y*y) + z*z) widened to double; NaN fails every comparison"""
    x, y, z = (cloud[:, q].astype(F32) for q in range(3))
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.sqrt((x * x + y * y) + z * z).astype(np.float64)
        zz = z.astype(np.float64)
        return (d > near) & (d < far) & (zz < z_high) & (zz > z_low)


def knn_d2_kdtree(xyz, k):
    o = R.RefAPDGICP(R.default_params())
    o.setInputTarget(np.ascontiguousarray(xyz[:, :3], dtype=F32))
    return o.knn_kdtree_batch("target", xyz[:, :3], k)[1]


def knn_d2_brute(xyz, k, chunk=256):
    """the k smallest fp32 squared distances of every point, FLANN L2_Simple: ((dx*dx) + dy*dy) + dz*dz, every step rounded to fp32"""
    p = np.ascontiguousarray(xyz[:, :3], dtype=F32)
    out = np.empty((len(p), k), dtype=F32)
    for a in range(0, len(p), chunk):
        q = p[a:a + chunk]
        dx, dy, dz = (q[:, None, c] - p[None, :, c] for c in range(3))
        d = dx * dx
        d = d + dy * dy
        d = d + dz * dz
        assert d.dtype == F32
        out[a:a + chunk] = np.sort(np.partition(d, k - 1, axis=1)[:, :k], axis=1)
    return out


def np_statistical(d2, mean_k, stddev_mul):
    """pcl::StatisticalOutlierRemoval::applyFilterIndices on rank-ordered fp32 squared distances [n, >= mean_k + 1] (rank 0: the point itself)"""
    acc = np.zeros(len(d2), dtype=np.float64)
    for r in range(1, mean_k + 1):
        acc = acc + np.sqrt(d2[:, r].astype(F32)).astype(np.float64)   # std::sqrt(float), double sum in rank order
    score = (acc / mean_k).astype(F32)
    n = len(score)
    s = float(np.cumsum(score.astype(np.float64))[-1])                 # (cumsum adds one after the other, np.sum pairwise)
    sq = float(np.cumsum((score * score).astype(np.float64))[-1])      # fp32 product, double sum
    mean = s / n
    var = (sq - s * s / n) / (n - 1)
    stddev = float(np.sqrt(var))
    thr = mean + stddev_mul * stddev
    return score, mean, stddev, thr, score.astype(np.float64) <= thr


def np_radius(d2, min_neighbors, radius):
    stat = d2[:, min_neighbors].astype(F32)
    return stat, stat.astype(np.float64) <= radius * radius
