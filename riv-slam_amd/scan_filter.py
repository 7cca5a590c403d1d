"""Scan preprocessing on the GPU: what PreprocessingNodelet::cloud_callback does to every scan before it becomes a registration
source (radar_graph_slam/apps/preprocessing_nodelet.cpp:812-815) -- distance_filter (:881-889), downsample
(:850-866, pcl::VoxelGrid or pcl::ApproximateVoxelGrid) and outlier_removal (:868-879, pcl::StatisticalOutlierRemoval / pcl::RadiusOutlierRemoval) -- with the
scan entering the device once and leaving as the device-resident cloud setInputSource accepts.  Host side of
include/apdgicp_hip.h's apdgicp_scan_filter_* entry points.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .registration import DevicePoints, _check, _cloud_arg, _ptr, load_library

OUTLIER_NONE, OUTLIER_STATISTICAL, OUTLIER_RADIUS = 0, 1, 2
_METHODS = {"NONE": OUTLIER_NONE, "STATISTICAL": OUTLIER_STATISTICAL, "RADIUS": OUTLIER_RADIUS}
DOWNSAMPLE_VOXELGRID, DOWNSAMPLE_APPROX_VOXELGRID = 0, 1
_DOWNSAMPLE_METHODS = {"VOXELGRID": DOWNSAMPLE_VOXELGRID, "APPROX_VOXELGRID": DOWNSAMPLE_APPROX_VOXELGRID}


def downsample_method_number(method) -> int:
    """apdgicp_downsample_method of a name ("VOXELGRID" / "APPROX_VOXELGRID") or a number (passed on: the library checks it)"""
    return _DOWNSAMPLE_METHODS[method.upper()] if isinstance(method, str) else int(method)


class ScanFilterParams(C.Structure):
    """apdgicp_scan_filter_params (include/apdgicp_hip.h)."""
    _fields_ = [
        ("use_distance_filter", C.c_int32),
        ("outlier_method", C.c_int32),
        ("mean_k", C.c_int32),
        ("min_neighbors", C.c_int32),
        ("near", C.c_double),
        ("far", C.c_double),
        ("z_low", C.c_double),
        ("z_high", C.c_double),
        ("stddev_mul", C.c_double),
        ("radius", C.c_double),
        ("leaf", C.c_float * 3),
        ("downsample_method", C.c_int32),
    ]


def default_filter_params(**kw) -> ScanFilterParams:
    """The nodelet's defaults (preprocessing_nodelet.cpp:137-205): gate 1 .. 100 m / -5 .. 20 m, VOXELGRID 0.1, STATISTICAL 20 / 1.0
    (RADIUS: 0.8 / 2).  leaf: a float, three floats or None (no downsampling); outlier_method: a name or a number;
    downsample_method: "VOXELGRID" (the default), "APPROX_VOXELGRID" or a number."""
    p = ScanFilterParams()
    load_library().apdgicp_scan_filter_default_params(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        if k == "leaf":
            v = (C.c_float * 3)(*(np.broadcast_to(np.asarray(0.0 if v is None else v, dtype=np.float32), (3,)).tolist()))
        elif k == "outlier_method" and isinstance(v, str):
            v = _METHODS[v.upper()]
        elif k == "downsample_method":
            v = downsample_method_number(v)
        setattr(p, k, v)
    return p


class ScanFilter:
    def __init__(self, params: ScanFilterParams | None = None, device: int = 0, stream=None, **kw):
        self.L = load_library()
        self.h = C.c_void_p()
        self.params = params if params is not None else default_filter_params(**kw)
        _check(self.L.apdgicp_scan_filter_create(C.byref(self.params), device, C.c_void_p(stream) if stream else None, C.byref(self.h)))
        self.n = 0

    def __del__(self):
        try:
            if self.h:
                self.L.apdgicp_scan_filter_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def set_params(self, params: ScanFilterParams | None = None, **kw):
        if params is None:
            params = ScanFilterParams.from_buffer_copy(self.params)
            d = default_filter_params(**kw)  # (converts leaf / the method's name)
            for k in kw:
                setattr(params, k, getattr(d, k))
        _check(self.L.apdgicp_scan_filter_set_params(self.h, C.byref(params)))
        self.params = params

    def run(self, cloud, intensity_column: int | None = 3) -> int:
        """cloud: [n, >=3] float32 (numpy, a torch CPU / CUDA tensor, DevicePoints); intensity_column: the column that holds the
        intensity (None, or a column the cloud does not have: 0 is kept).  Returns the number of points of the filtered scan."""
        ptr, n, stride, dev, keep = _cloud_arg(cloud)
        if dev and hasattr(keep, "data_ptr"):
            import torch
            torch.cuda.current_stream(keep.device).synchronize()  # the tensor's producer; the filter runs on a stream of its own
        ioff = -1
        if intensity_column is not None and 4 * (intensity_column + 1) <= stride:
            ioff = 4 * intensity_column
        n_out = C.c_int64()
        self.n = 0
        _check(self.L.apdgicp_scan_filter_run(self.h, ptr, n, stride, ioff, dev, C.byref(n_out)))
        self.n = n_out.value
        return self.n

    def points(self) -> DevicePoints:
        """the filtered scan in device memory ({x, y, z, intensity}, 16-byte stride), valid until the next run"""
        p, n = C.c_void_p(), C.c_int64()
        _check(self.L.apdgicp_scan_filter_points(self.h, C.byref(p), C.byref(n)))
        return DevicePoints(p.value or 0, n.value, 16, owner=self)

    def to_numpy(self) -> np.ndarray:
        out = np.empty((self.n, 4), dtype=np.float32)
        if self.n:
            _check(self.L.apdgicp_scan_filter_copy(self.h, _ptr(out), self.n, 0))
        return out

    def stage_counts(self):
        """(input, behind the range gate, behind downsample, output) of the last run"""
        c = (C.c_int64 * 4)()
        _check(self.L.apdgicp_scan_filter_stage_counts(self.h, c))
        return tuple(int(v) for v in c)

    def scores(self):
        """What the outlier filter of the last run decided on, in the order of the downsampled cloud: dict(stat = the mean distance to
        the mean_k nearest neighbours (STATISTICAL) or d2[min_neighbors] (RADIUS), kept = bool mask, mean, stddev, thr)."""
        n = self.stage_counts()[2] if self.params.outlier_method != OUTLIER_NONE else 0
        stat = np.empty(n, dtype=np.float32)
        kept = np.empty(n, dtype=np.uint8)
        m, s, t = C.c_double(), C.c_double(), C.c_double()
        _check(self.L.apdgicp_scan_filter_scores(self.h, _ptr(stat), _ptr(kept), n, C.byref(m), C.byref(s), C.byref(t)))
        return dict(stat=stat, kept=kept.astype(bool), mean=m.value, stddev=s.value, thr=t.value)


def preprocess_and_set_source(registration, raw_cloud, filter: ScanFilter, intensity_column: int | None = 3) -> int:
    """cloud_callback's three filters (:812-815) followed by the odometry's setInputSource on the published cloud
    (scan_matching_odometry_nodelet.cpp:437-482), without the scan leaving the device in between.  Returns the filtered size
    (0: nothing is set)."""
    n = filter.run(raw_cloud, intensity_column)
    if n:
        registration.setInputSource(filter.points())
    return n
