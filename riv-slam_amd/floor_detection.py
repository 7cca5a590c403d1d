"""Floor plane detection and under-floor removal on the GPU: radar_graph_slam::FloorDetectionNodelet
(radar_graph_slam/apps/floor_detection_nodelet.cpp), which runs on every raw scan at the launch defaults: its coefficients become the
ground-plane factor of every keyframe (radar_graph_slam_nodelet.cpp:273, 448-460), its under-floor-clipped cloud is published for the
rest of the chain.  Host side of include/apdgicp_hip.h's apdgicp_floor_* entry points.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .registration import DevicePoints, _check, _cloud_arg, _ptr, load_library

REJECT = {0: "detected", 1: "too few points for RANSAC", 2: "no model", 3: "too few inliers", 4: "the detected floor is not horizontal"}


class FloorParams(C.Structure):
    """apdgicp_floor_params (include/apdgicp_hip.h): the nodelet's eight parameters, RANSAC's three, normal_k and n_hypotheses."""
    _fields_ = [(name, C.c_double) for name in (
        "tilt_deg", "sensor_height", "height_clip_range", "floor_normal_thresh", "normal_filter_thresh", "floor_tolerance", "distance_threshold",
        "probability")] + [(name, C.c_int32) for name in (
            "floor_pts_thresh", "use_normal_filtering", "max_iterations", "normal_k", "n_hypotheses")] + [("reserved", C.c_int32 * 3)]


class FloorResult(C.Structure):
    """apdgicp_floor_result (include/apdgicp_hip.h)."""
    _fields_ = [("coeffs", C.c_float * 4), ("raw_coeffs", C.c_float * 4)] + [(name, C.c_int32) for name in (
        "detected", "ground_initialized", "reject_reason", "n_input", "n_clipped", "n_filtered", "n_inliers", "n_under_floor", "iterations", "skipped", "winner",
        "table_exhausted", "K")] + [("reserved", C.c_int32 * 3)]


assert C.sizeof(FloorParams) == 96 and C.sizeof(FloorResult) == 96


def default_floor_params(**kw) -> FloorParams:
    """initialize_params() of the nodelet (floor_detection_nodelet.cpp:62-70), its RANSAC threshold (:185), pcl::SampleConsensus's
    probability / max_iterations, k = 10 of normal_filtering (:288); n_hypotheses = 64"""
    p = FloorParams()
    load_library().apdgicp_floor_default_params(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


class FloorDetector:
    def __init__(self, params: FloorParams | None = None, device: int = 0, stream=None, **kw):
        self.L = load_library()
        self.h = C.c_void_p()
        self.params = params if params is not None else default_floor_params(**kw)
        _check(self.L.apdgicp_floor_create(C.byref(self.params), device, C.c_void_p(stream) if stream else None, C.byref(self.h)))
        self.result = FloorResult()
        self.n = 0

    def __del__(self):
        try:
            if self.h:
                self.L.apdgicp_floor_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def set_params(self, params: FloorParams | None = None, **kw):
        """the callback's memory is kept (reset() restores it)"""
        if params is None:
            params = FloorParams.from_buffer_copy(self.params)
            for k, v in kw.items():
                if not hasattr(params, k):
                    raise AttributeError(k)
                setattr(params, k, v)
        _check(self.L.apdgicp_floor_set_params(self.h, C.byref(params)))
        self.params = params

    def reset(self):
        """prev_coeffs = (0, 0, 0, sensor_height - height_clip_range), ground_intialized = false (:75-80)"""
        _check(self.L.apdgicp_floor_reset(self.h))

    def run(self, scan, words=None, seed: int = 0, intensity_column: int = 3) -> FloorResult:
        """scan: [n, >=3] float32 {x, y, z, intensity} (numpy, a torch CPU / CUDA tensor, DevicePoints; intensity_column < 0 or a scan
        without that column: intensity 0).  words: [K, 3] uint32, the random draws of the RANSAC (default:
        numpy.random.default_rng(seed).integers(0, 2**32, (K, 3), dtype=uint32)).  result.table_exhausted: supply more words."""
        ptr, n, stride, dev, keep = _cloud_arg(scan)
        if dev and hasattr(keep, "data_ptr"):
            import torch
            torch.cuda.current_stream(keep.device).synchronize()  # the tensor's producer; the detector runs on a stream of its own
        K = self.params.n_hypotheses
        if words is None:
            words = np.random.default_rng(seed).integers(0, 2**32, (K, 3), dtype=np.uint32)
        words = np.ascontiguousarray(words, dtype=np.uint32)
        if n == 0:
            stride = 16
        ioff = 4 * intensity_column if intensity_column >= 0 and 4 * intensity_column + 4 <= stride else -1
        self.n = 0
        res = FloorResult()
        _check(self.L.apdgicp_floor_run(self.h, ptr, n, stride, ioff, dev, _ptr(words), words.size, C.byref(res)))
        self.result, self.n = res, n
        return res

    def _cloud(self, f) -> DevicePoints:
        p, n = C.c_void_p(), C.c_int64()
        _check(f(self.h, C.byref(p), None, C.byref(n)))
        return DevicePoints(p.value or 0, n.value, 16, owner=self)

    def inlier_cloud(self) -> DevicePoints:
        """floor_points (:215-222) of the last run in device memory ({x, y, z, intensity}, 16-byte stride), valid until the next run;
        empty unless a floor was detected"""
        return self._cloud(self.L.apdgicp_floor_inliers)

    def under_floor_filtered(self) -> DevicePoints:
        """/underfloor_filtered_points (:132-137) of the last run in device memory: what ScanFilter.run and setInputSource accept"""
        return self._cloud(self.L.apdgicp_floor_under_floor_filtered)

    def to_numpy(self, which: str = "inliers") -> dict:
        """dict(xyzi [k, 4] fp32, index [k] int32 into the scan) of "clipped" (tilted frame), "filtered", "inliers" or "under_floor" """
        w = {"clipped": 0, "filtered": 1, "inliers": 2, "under_floor": 3}[which]
        r = self.result
        k = (r.n_clipped, r.n_filtered, self.inlier_cloud().n, r.n_under_floor)[w]
        out = dict(xyzi=np.empty((k, 4), dtype=np.float32), index=np.empty(k, dtype=np.int32))
        if k:
            _check(self.L.apdgicp_floor_copy(self.h, w, _ptr(out["xyzi"]), _ptr(out["index"]), k))
        return out

    def hypotheses(self):
        """(coeffs [K, 4] float32, bad [K] bool, n_in [K] int32) of the last run's hypotheses"""
        K = self.result.K
        coeffs, bad, n_in = np.zeros((K, 4), dtype=np.float32), np.zeros(K, dtype=np.uint8), np.zeros(K, dtype=np.int32)
        if K:
            _check(self.L.apdgicp_floor_hypotheses(self.h, _ptr(coeffs), _ptr(bad), _ptr(n_in), K))
        return coeffs, bad.astype(bool), n_in

    def debug(self) -> dict:
        """the intermediate results of the last run: clip_mask [n] bool, normal_stat [n_clipped] float32 (NaN unless the search ran),
        samples [K, 3] int32 (-1 when RANSAC did not run)"""
        r = self.result
        mask, stat = np.zeros(self.n, dtype=np.uint8), np.full(r.n_clipped, np.nan, dtype=np.float32)
        samples = np.full((r.K, 3), -1, dtype=np.int32)
        _check(self.L.apdgicp_floor_debug(self.h, _ptr(mask), mask.size, _ptr(stat), stat.size, _ptr(samples), samples.size))
        return dict(clip_mask=mask.astype(bool), normal_stat=stat, samples=samples)
