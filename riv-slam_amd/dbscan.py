"""DBSCAN clustering on the GPU: DBSCANSimpleCluster::extract (radar_graph_slam/include/dbscan/DBSCAN_simple.h), the clustering of the
moving points that the ego-velocity estimate rejects into objects with a centre, an extent and a radial speed.  Host side of
include/apdgicp_hip.h's apdgicp_dbscan_* entry points; the semantics are D1 .. D7 there.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .registration import DevicePoints, _check, _cloud_arg, _ptr, load_library


class DBSCANParams(C.Structure):
    """apdgicp_dbscan_params (include/apdgicp_hip.h)."""
    _fields_ = [("eps", C.c_double), ("min_pts", C.c_int32), ("min_cluster_size", C.c_int32), ("max_cluster_size", C.c_int32), ("reserved", C.c_int32)]


# apdgicp_dbscan_cluster (include/apdgicp_hip.h): one row of the table
CLUSTER_DTYPE = np.dtype([("centroid", np.float64, 3), ("doppler_mean", np.float64), ("min", np.float32, 3), ("max", np.float32, 3), ("doppler_min", np.float32),
                          ("doppler_max", np.float32), ("seed", np.int32), ("size", np.int32), ("n_core", np.int32), ("reserved", np.int32)])

assert C.sizeof(DBSCANParams) == 24 and CLUSTER_DTYPE.itemsize == 80


def default_dbscan_params(**kw) -> DBSCANParams:
    """The reference's defaults (DBSCAN_simple.h:111-114): eps 0 (a run is refused until it is set), minPts 1, cluster sizes 1 .. INT_MAX."""
    p = DBSCANParams()
    load_library().apdgicp_dbscan_default_params(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def _lane_arg(lane, n: int):
    """-> (pointer, stride_bytes, on_device, keepalive) of one float per point: numpy [n], a torch tensor [n], or (device pointer, stride_bytes)"""
    if lane is None:
        return None, 0, None, None
    if isinstance(lane, tuple):
        return C.c_void_p(int(lane[0])), int(lane[1]), 1, lane
    if hasattr(lane, "data_ptr"):
        if lane.dim() != 1 or lane.shape[0] != n or str(lane.dtype) != "torch.float32":
            raise ValueError("doppler tensor must be [n] float32")
        return C.c_void_p(lane.data_ptr()), lane.stride(0) * 4 if n > 1 else 4, 1 if lane.is_cuda else 0, lane
    a = np.ascontiguousarray(lane, dtype=np.float32)
    if a.shape != (n,):
        raise ValueError("doppler must be [n]")
    return _ptr(a), 4, 0, a


class DBSCAN:
    """DBSCANSimpleCluster's surface: the four setters, then extract(cloud)."""

    def __init__(self, params: DBSCANParams | None = None, device: int = 0, stream=None, **kw):
        self.L = load_library()
        self.h = C.c_void_p()
        self.params = params if params is not None else default_dbscan_params(**kw)
        _check(self.L.apdgicp_dbscan_create(C.byref(self.params), device, C.c_void_p(stream) if stream else None, C.byref(self.h)))
        self.n = self.n_clusters = 0

    def __del__(self):
        try:
            if self.h:
                self.L.apdgicp_dbscan_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def set_params(self, **kw):
        params = DBSCANParams.from_buffer_copy(self.params)
        for k, v in kw.items():
            if not hasattr(params, k):
                raise AttributeError(k)
            setattr(params, k, v)
        _check(self.L.apdgicp_dbscan_set_params(self.h, C.byref(params)))
        self.params = params

    def setClusterTolerance(self, tolerance: float):
        self.set_params(eps=float(tolerance))

    def setCorePointMinPts(self, min_pts: int):
        self.set_params(min_pts=int(min_pts))

    def setMinClusterSize(self, n: int):
        self.set_params(min_cluster_size=int(n))

    def setMaxClusterSize(self, n: int):
        self.set_params(max_cluster_size=int(n))

    def setSearchMethod(self, tree=None):  # accepted and ignored: the search is the device grid
        pass

    def run(self, cloud, doppler=None) -> int:
        """cloud: [n, >=3] float32 (numpy, a torch CPU / CUDA tensor, DevicePoints); doppler: one float per point in the same memory space
        (numpy / tensor [n], or (device pointer, stride_bytes)), or None.  Returns the number of kept clusters."""
        ptr, n, stride, dev, keep = _cloud_arg(cloud)
        dptr, dstride, ddev, dkeep = _lane_arg(doppler, n)
        if doppler is not None and n and ddev != dev:
            raise ValueError("cloud and doppler must both be on the device or both on the host")
        for k in (keep, dkeep):
            if dev and hasattr(k, "data_ptr"):
                import torch
                torch.cuda.current_stream(k.device).synchronize()  # the tensor's producer; the clustering runs on a stream of its own
        if n == 0:  # (an empty array has no meaningful strides)
            stride, dstride = 12, 4
        K = C.c_int32()
        self.n = self.n_clusters = 0
        _check(self.L.apdgicp_dbscan_run(self.h, ptr, n, stride, dptr, dstride, dev, C.byref(K)))
        self.n, self.n_clusters = n, K.value
        return K.value

    def extract(self, cloud, doppler=None) -> list:
        """extract(cluster_indices): the member lists, largest cluster first, each in ascending index"""
        self.run(cloud, doppler)
        off, idx = self.members()
        return [idx[off[r]:off[r + 1]] for r in range(self.n_clusters)]

    def labels_device(self) -> tuple[int, int]:
        """(device pointer to n int32 labels, n), valid until the next run"""
        p, n = C.c_void_p(), C.c_int64()
        _check(self.L.apdgicp_dbscan_labels(self.h, C.byref(p), C.byref(n)))
        return p.value or 0, n.value

    def labels(self) -> np.ndarray:
        """int32 per point: the rank of its kept primary cluster, or -1"""
        out = np.empty(self.n, dtype=np.int32)
        if self.n:
            _check(self.L.apdgicp_dbscan_copy_labels(self.h, _ptr(out), self.n))
        return out

    def clusters(self) -> np.ndarray:
        """the table, one CLUSTER_DTYPE row per kept cluster in rank order"""
        out = np.zeros(self.n_clusters, dtype=CLUSTER_DTYPE)
        if self.n_clusters:
            _check(self.L.apdgicp_dbscan_clusters(self.h, _ptr(out), self.n_clusters))
        return out

    def members(self) -> tuple[np.ndarray, np.ndarray]:
        """(offsets [K + 1], indices [offsets[K]]): the member lists as CSR (a point of D5 is listed by two clusters)"""
        off, m = np.zeros(self.n_clusters + 1, dtype=np.int32), C.c_int64()
        _check(self.L.apdgicp_dbscan_members(self.h, _ptr(off), off.size, None, 0, C.byref(m)))
        idx = np.empty(m.value, dtype=np.int32)
        if m.value:
            _check(self.L.apdgicp_dbscan_members(self.h, None, 0, _ptr(idx), idx.size, None))
        return off, idx

    def debug(self) -> dict:
        """before the size filter: cnt (D2), core, root (a core point's seed, else -1), primary (D4: seed of the primary cluster, -1 noise)"""
        n = self.n
        d = dict(cnt=np.zeros(n, dtype=np.int32), core=np.zeros(n, dtype=np.uint8), root=np.full(n, -1, dtype=np.int32), primary=np.full(n, -1, dtype=np.int32))
        if n:
            _check(self.L.apdgicp_dbscan_debug(self.h, _ptr(d["cnt"]), _ptr(d["core"]), _ptr(d["root"]), _ptr(d["primary"]), n))
        d["core"] = d["core"].astype(bool)
        return d

    def set_profiling(self, on: bool = True):
        """events at the phase boundaries of every run (one more wait per run): stats() then carries the device time of each phase"""
        _check(self.L.apdgicp_dbscan_set_profiling(self.h, 1 if on else 0))

    def stats(self) -> dict:
        """launches and waits of the last run; phase_ms = {sort, count, union_flatten, border, output} when profiling is on (else zeros)"""
        a, b, ph = C.c_int64(), C.c_int64(), (C.c_double * 5)()
        _check(self.L.apdgicp_dbscan_stats(self.h, C.byref(a), C.byref(b), ph))
        return dict(launches=a.value, waits=b.value, phase_ms=dict(zip(("sort", "count", "union_flatten", "border", "output"), (float(v) for v in ph))))


def cluster_moving_points(ego, dbscan: DBSCAN, scan_filter=None) -> int:
    """Moving objects from the last run of an EgoVelocityEstimator: its outlier cloud (apdgicp_ego_velocity_outliers: device xyzi and Doppler)
    goes to dbscan.run as device pointers -- no point visits the host.  With `scan_filter` (a ScanFilter set to OUTLIER_RADIUS, gate off, no
    leaf) the radius filter of preprocessing_nodelet.cpp:766-774 runs first, as there only when the cloud has more than 3 points; its output
    is {x, y, z, intensity} like the reference's, so the clustered cloud then has no Doppler lane (the table's Doppler columns are 0) and
    its indices are those of the filtered cloud.  Returns the number of kept clusters; labels, table and members are dbscan's."""
    xyzi, dop, n = C.c_void_p(), C.c_void_p(), C.c_int64()
    _check(ego.L.apdgicp_ego_velocity_outliers(ego.h, C.byref(xyzi), C.byref(dop), None, C.byref(n)))
    cloud = DevicePoints(xyzi.value or 0, n.value, 16, owner=ego)
    if scan_filter is not None and n.value > 3:
        kept = scan_filter.run(cloud)
        return dbscan.run(scan_filter.points() if kept else np.zeros((0, 3), dtype=np.float32))
    if n.value == 0:
        return dbscan.run(np.zeros((0, 3), dtype=np.float32))
    return dbscan.run(cloud, (dop.value, 4))
