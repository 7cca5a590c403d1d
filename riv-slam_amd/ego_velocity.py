"""Doppler ego-velocity estimation and moving-point removal on the GPU: rio::RadarEgoVelocityEstimator::estimate
(radar_graph_slam/src/radar_ego_velocity_estimator.cpp), the step PreprocessingNodelet::cloud_callback runs on the raw
{x, y, z, intensity, doppler} scan right before its three filters (radar_graph_slam/apps/preprocessing_nodelet.cpp:708-741).  Its output
is the sensor velocity with sigmas (the twist the graph consumes) and the inlier cloud, which replaces the raw scan as src_cloud when
enable_dynamic_object_removal is set (:775-786).  Host side of include/apdgicp_hip.h's apdgicp_ego_velocity_* entry points.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .registration import DevicePoints, _check, _cloud_arg, _ptr, load_library
from .scan_filter import ScanFilter


class EgoVelocityParams(C.Structure):
    """apdgicp_ego_velocity_params (include/apdgicp_hip.h): every field of RadarEgoVelocityEstimatorConfig + n_hypotheses."""
    _fields_ = [(name, C.c_float) for name in (
        "min_dist", "max_dist", "min_db", "elevation_thresh_deg", "azimuth_thresh_deg", "doppler_velocity_correction_factor",
        "thresh_zero_velocity", "allowed_outlier_percentage", "sigma_zero_velocity_x", "sigma_zero_velocity_y", "sigma_zero_velocity_z",
        "sigma_offset_radar_x", "sigma_offset_radar_y", "sigma_offset_radar_z", "max_sigma_x", "max_sigma_y", "max_sigma_z", "max_r_cond",
        "outlier_prob", "success_prob", "inlier_thresh")] + [(name, C.c_int32) for name in (
            "use_cholesky_instead_of_bdcsvd", "use_ransac", "N_ransac_points", "n_hypotheses", "reserved")]


class EgoVelocityResult(C.Structure):
    """apdgicp_ego_velocity_result (include/apdgicp_hip.h)."""
    _fields_ = [("v", C.c_double * 3), ("sigma", C.c_double * 3)] + [(name, C.c_int32) for name in (
        "success", "zero_velocity", "sigma_in_bounds", "m", "n_inlier", "n_outlier", "best_in", "best_out", "K", "reserved")]


assert C.sizeof(EgoVelocityParams) == 26 * 4 and C.sizeof(EgoVelocityResult) == 88


def default_ego_velocity_params(**kw) -> EgoVelocityParams:
    """RadarEgoVelocityEstimatorConfig's defaults (radar_ego_velocity_estimator.h:30-60); n_hypotheses = 0: setRansacIter's formula."""
    p = EgoVelocityParams()
    load_library().apdgicp_ego_velocity_default_params(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def hypothesis_count(params: EgoVelocityParams) -> int:
    """ransac_iter_ of these parameters (setRansacIter, radar_ego_velocity_estimator.h:138-143), or n_hypotheses; 0 without RANSAC"""
    if not params.use_ransac:
        return 0
    k = C.c_int32()
    _check(load_library().apdgicp_ego_velocity_hypothesis_count(C.byref(params), C.byref(k)))
    return k.value


class EgoVelocityEstimator:
    def __init__(self, params: EgoVelocityParams | None = None, device: int = 0, stream=None, **kw):
        self.L = load_library()
        self.h = C.c_void_p()
        self.params = params if params is not None else default_ego_velocity_params(**kw)
        _check(self.L.apdgicp_ego_velocity_create(C.byref(self.params), device, C.c_void_p(stream) if stream else None, C.byref(self.h)))
        self.result = EgoVelocityResult()
        self.n = 0

    def __del__(self):
        try:
            if self.h:
                self.L.apdgicp_ego_velocity_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def set_params(self, params: EgoVelocityParams | None = None, **kw):
        if params is None:
            params = EgoVelocityParams.from_buffer_copy(self.params)
            for k, v in kw.items():
                if not hasattr(params, k):
                    raise AttributeError(k)
                setattr(params, k, v)
        _check(self.L.apdgicp_ego_velocity_set_params(self.h, C.byref(params)))
        self.params = params

    def run(self, cloud, words=None, seed: int = 0, intensity_column: int = 3, doppler_column: int = 4) -> EgoVelocityResult:
        """cloud: [n, >=5] float32 {x, y, z, intensity, doppler} (numpy, a torch CPU / CUDA tensor, DevicePoints).  words: [K, S] uint32,
        the random draws of the RANSAC (default: numpy.random.default_rng(seed).integers(0, 2**32, (K, S), dtype=uint32))."""
        ptr, n, stride, dev, keep = _cloud_arg(cloud)
        if dev and hasattr(keep, "data_ptr"):
            import torch
            torch.cuda.current_stream(keep.device).synchronize()  # the tensor's producer; the estimator runs on a stream of its own
        K, S = hypothesis_count(self.params), self.params.N_ransac_points
        if words is None:
            words = np.random.default_rng(seed).integers(0, 2**32, (K, S), dtype=np.uint32)
        words = np.ascontiguousarray(words, dtype=np.uint32)
        if n == 0:  # (an empty array has no meaningful strides)
            stride = 4 * (max(intensity_column, doppler_column) + 1)
        self.n = 0
        res = EgoVelocityResult()
        _check(self.L.apdgicp_ego_velocity_run(self.h, ptr, n, stride, 4 * intensity_column, 4 * doppler_column, dev, _ptr(words), words.size, C.byref(res)))
        self.result, self.n = res, n
        return res

    def _cloud(self, which: int) -> DevicePoints:
        p, n = C.c_void_p(), C.c_int64()
        f = self.L.apdgicp_ego_velocity_outliers if which else self.L.apdgicp_ego_velocity_inliers
        _check(f(self.h, C.byref(p), None, None, C.byref(n)))
        return DevicePoints(p.value or 0, n.value, 16, owner=self)

    def inliers(self) -> DevicePoints:
        """the static points of the last run in device memory ({x, y, z, intensity}, 16-byte stride), valid until the next run"""
        return self._cloud(0)

    def outliers(self) -> DevicePoints:
        """the moving points of the last run (the best outlier list), like inliers()"""
        return self._cloud(1)

    def to_numpy(self, which: str = "inliers") -> dict:
        """dict(xyzi [k, 4] fp32, doppler [k] fp32, index [k] int32 into the scan, row [k] int32 into the valid rows) of one cloud"""
        w = {"inliers": 0, "outliers": 1}[which]
        k = self.result.n_outlier if w else self.result.n_inlier
        out = dict(xyzi=np.empty((k, 4), dtype=np.float32), doppler=np.empty(k, dtype=np.float32), index=np.empty(k, dtype=np.int32), row=np.empty(k, dtype=np.int32))
        if k:
            _check(self.L.apdgicp_ego_velocity_copy(self.h, w, _ptr(out["xyzi"]), _ptr(out["doppler"]), _ptr(out["index"]), _ptr(out["row"]), k))
        return out

    def hypotheses(self):
        """(v_k [K, 3] float64, n_in [K] int32) of the last run's hypotheses (n_in: before the 5 % rule)"""
        K = self.result.K
        vk, n_in = np.zeros((K, 3), dtype=np.float64), np.zeros(K, dtype=np.int32)
        if K:
            _check(self.L.apdgicp_ego_velocity_hypotheses(self.h, _ptr(vk), _ptr(n_in), K))
        return vk, n_in

    def debug(self) -> dict:
        """the intermediate results of the last run: valid [n] bool, rows [m, 4] float64, samples [K, S] int32, selected_abs_v"""
        m, K, S = self.result.m, self.result.K, self.params.N_ransac_points
        valid, rows = np.zeros(self.n, dtype=np.uint8), np.zeros((m, 4), dtype=np.float64)
        samples, sel = np.full((K, S), -1, dtype=np.int32), C.c_float()
        _check(self.L.apdgicp_ego_velocity_debug(self.h, _ptr(valid), valid.size, _ptr(rows), m, _ptr(samples), samples.size, C.byref(sel)))
        return dict(valid=valid.astype(bool), rows=rows, samples=samples, selected_abs_v=sel.value)


def estimate_filter_and_set_source(registration, raw, estimator: EgoVelocityEstimator, scan_filter: ScanFilter, enable_dynamic_object_removal: bool = False,
                                   words=None, seed: int = 0) -> tuple[EgoVelocityResult, int]:
    """cloud_callback from the ego-velocity estimate to the published cloud (preprocessing_nodelet.cpp:708-815) followed by the odometry's
    setInputSource: `raw` ([n, >=5] {x, y, z, intensity, doppler}) crosses to the device once; the estimator's inlier cloud
    (enable_dynamic_object_removal, :775-786) or the raw {x, y, z, intensity} is handed to ScanFilter.run as a device cloud.  Returns
    (the estimate, the filtered size); nothing is set when the filtered scan is empty."""
    dev_raw, keep = raw, None
    if not isinstance(raw, DevicePoints) and not getattr(raw, "is_cuda", False):
        import torch
        keep = torch.from_numpy(np.ascontiguousarray(raw, dtype=np.float32)) if not hasattr(raw, "data_ptr") else raw
        dev_raw = keep.cuda()
    res = estimator.run(dev_raw, words=words, seed=seed)
    if enable_dynamic_object_removal:
        cloud = estimator.inliers()
        n = scan_filter.run(cloud) if cloud.n else 0
    else:
        n = scan_filter.run(dev_raw)
    if n:
        registration.setInputSource(scan_filter.points())
    return res, n
