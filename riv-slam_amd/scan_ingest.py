"""Scan ingest and deskew on the GPU: the two ends of PreprocessingNodelet::cloud_callback
(radar_graph_slam/apps/preprocessing_nodelet.cpp) -- the power gate and the packing of the message's arrays into the
{x, y, z, intensity, doppler} cloud the ego-velocity estimate reads (:667-697, :497-506), and the IMU deskew with the base-link
transform between that estimate and distance_filter (:792-810, :914-975).  Host side of include/apdgicp_hip.h's apdgicp_scan_ingest_*
entry points; the semantics are I1 .. I7 there.  preprocess_scan() is the whole callback with every per-point step on the device.
run_polar() is the head of cloud_callback_scan (:324-340, PI1 .. PI5: a RadarScanExtended of range / azimuth / elevation targets),
preprocess_polar_scan() that callback, and histogram_*() the distance histogram that ends all three (:451-461, H1 .. H4).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .registration import DevicePoints, _check, _cloud_arg, _ptr, load_library

FLAG_XF_LINEAR_CHAIN = 2
MAX_POINTS = 1 << 24
HISTOGRAM_BINS = 100
POLAR_LANES = ("range", "azimuth", "elevation", "snr", "velocity")                      # the order of apdgicp_scan_ingest_run_polar's lanes
TARGET_COLUMN = dict(range=0, azimuth=1, elevation=2, velocity=3, snr=4)                # their places among the 19 floats of a RadarTargetExtended


class ScanIngestParams(C.Structure):
    """apdgicp_scan_ingest_params (include/apdgicp_hip.h)."""
    _fields_ = [("power_threshold", C.c_float), ("gate", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32)]


assert C.sizeof(ScanIngestParams) == 16


def default_ingest_params(**kw) -> ScanIngestParams:
    """power_threshold 0 (preprocessing_nodelet.cpp:107), gate on, the pairwise fp32 order"""
    p = ScanIngestParams()
    load_library().apdgicp_scan_ingest_default_params(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def _lane_arg(lane, n: int):
    """-> (pointer, stride_bytes, on_device, keepalive) of one float per point, strides kept: numpy [n] (any stride that is a multiple of
    4 bytes), a torch CPU / CUDA tensor [n], or (device pointer, stride_bytes)"""
    if isinstance(lane, tuple):
        return C.c_void_p(int(lane[0])), int(lane[1]), 1, lane
    if hasattr(lane, "data_ptr"):
        if lane.dim() != 1 or lane.shape[0] != n or str(lane.dtype) != "torch.float32":
            raise ValueError("a lane tensor must be [n] float32")
        return C.c_void_p(lane.data_ptr()), lane.stride(0) * 4 if n > 1 else 4, 1 if lane.is_cuda else 0, lane
    a = np.asarray(lane)
    if a.dtype != np.float32 or a.ndim != 1 or (n > 1 and (a.strides[0] < 4 or a.strides[0] % 4)):
        a = np.ascontiguousarray(a, dtype=np.float32)
    if a.shape != (n,):
        raise ValueError("a lane must be [n]")
    return _ptr(a), a.strides[0] if n > 1 else 4, 0, a


def _empty_as_numpy(cloud, width: int):
    """an empty cloud of any kind as an empty numpy array (an empty torch tensor has no strides to speak of)"""
    shape = getattr(cloud, "shape", None)
    if shape is not None and len(shape) == 2 and shape[0] == 0:
        return np.zeros((0, width), dtype=np.float32)
    return cloud


def _mat16(T):
    """a 4x4 as the column-major float[16] the C ABI reads, or None"""
    if T is None:
        return None
    m = np.asarray(T, dtype=np.float32)
    if m.shape != (4, 4):
        raise ValueError("a transform must be 4x4")
    return np.ascontiguousarray(m.T).reshape(16)


def _wait_for_producer(*keeps):
    for k in keeps:
        if hasattr(k, "data_ptr") and getattr(k, "is_cuda", False):
            import torch
            torch.cuda.current_stream(k.device).synchronize()  # the tensor's producer; the object runs on a stream of its own


class ScanIngest:
    def __init__(self, params: ScanIngestParams | None = None, device: int = 0, stream=None, **kw):
        self.L = load_library()
        self.h = C.c_void_p()
        self.params = params if params is not None else default_ingest_params(**kw)
        _check(self.L.apdgicp_scan_ingest_create(C.byref(self.params), device, C.c_void_p(stream) if stream else None, C.byref(self.h)))
        self.n = self.n_deskewed = 0

    def __del__(self):
        try:
            if self.h:
                self.L.apdgicp_scan_ingest_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def set_params(self, params: ScanIngestParams | None = None, **kw):
        if params is None:
            params = ScanIngestParams.from_buffer_copy(self.params)
            for k, v in kw.items():
                if not hasattr(params, k):
                    raise AttributeError(k)
                setattr(params, k, v)
        _check(self.L.apdgicp_scan_ingest_set_params(self.h, C.byref(params)))
        self.params = params

    def run(self, xyz, intensity, doppler, pre_transform=None) -> int:
        """xyz: [n, >=3] float32 (numpy, a torch CPU / CUDA tensor, DevicePoints; a strided view of an array of structures is read in
        place); intensity, doppler: one float per point in the same memory space (numpy / tensor [n], strided views likewise, or
        (device pointer, stride_bytes)); pre_transform: 4x4 or None.  Returns the number of rows."""
        ptr, n, stride, dev, keep = _cloud_arg(_empty_as_numpy(xyz, 3))
        if n == 0:
            intensity = doppler = np.zeros(0, dtype=np.float32)
        iptr, istride, idev, ikeep = _lane_arg(intensity, n)
        dptr, dstride, ddev, dkeep = _lane_arg(doppler, n)
        if n and not (dev == idev == ddev):
            raise ValueError("the three lanes must all be on the device or all on the host")
        if dev:
            _wait_for_producer(keep, ikeep, dkeep)
        if n == 0:  # (an empty array has no meaningful strides)
            stride, istride, dstride = 12, 4, 4
        m = _mat16(pre_transform)
        n_out = C.c_int64()
        self.n = 0
        _check(self.L.apdgicp_scan_ingest_run(self.h, ptr, n, stride, iptr, istride, dptr, dstride, dev, _ptr(m) if m is not None else None, C.byref(n_out)))
        self.n = n_out.value
        return self.n

    def run_polar(self, targets=None, **lanes) -> int:
        """One msgs_radar/RadarScanExtended (PI1 .. PI5).  targets: the RadarTargetExtended[] as [n, 19] float32 (numpy, a torch CPU / CUDA
        tensor; any [n, >= 5] array with range, azimuth, elevation, velocity, snr in columns 0 .. 4 is read in place), a numpy structured
        array with those five float32 fields, or DevicePoints of such records -- or, instead of `targets`, the five lanes by keyword
        (range=, azimuth=, elevation=, snr=, velocity=: numpy / tensor [n], strided views likewise, or (device pointer, stride_bytes)
        together with n=).  Every target becomes a row; does not wait.  Returns the number of rows (= n)."""
        n = lanes.pop("n", None)
        if targets is not None:
            if lanes:
                raise TypeError("either `targets` or the five lanes by keyword")
            if isinstance(targets, DevicePoints):
                n = targets.n
                lanes = {k: (targets.ptr + 4 * TARGET_COLUMN[k], targets.stride_bytes) for k in POLAR_LANES}
            elif getattr(getattr(targets, "dtype", None), "names", None):
                lanes = {k: targets[k] for k in POLAR_LANES}
            else:
                if not hasattr(targets, "data_ptr"):
                    targets = np.asarray(targets)
                    if targets.dtype != np.float32:
                        targets = np.ascontiguousarray(targets, dtype=np.float32)
                if len(targets.shape) != 2 or targets.shape[1] < 5:
                    raise ValueError("targets must be [n, >= 5]")
                lanes = {k: targets[:, TARGET_COLUMN[k]] for k in POLAR_LANES}
        if sorted(lanes) != sorted(POLAR_LANES):
            raise TypeError("run_polar needs range, azimuth, elevation, snr and velocity")
        if n is None:
            n = next(int(v.shape[0]) for v in lanes.values() if not isinstance(v, tuple))
        args = [_lane_arg(lanes[k], n) for k in POLAR_LANES]
        if n and len({a[2] for a in args}) != 1:
            raise ValueError("the five lanes must all be on the device or all on the host")
        dev = args[0][2]
        if dev:
            _wait_for_producer(*(a[3] for a in args))
        flat = []
        for ptr, stride, _, _ in args:
            flat += [ptr, stride if n else 4]
        n_out = C.c_int64()
        _check(self.L.apdgicp_scan_ingest_run_polar(self.h, *flat, n, dev, C.byref(n_out)))
        self.n = n_out.value
        return self.n

    def histogram_add(self, cloud) -> int:
        """one frame of the distance histogram (H1 .. H4) from a cloud ([n, >= 3] float32: numpy, a torch CPU / CUDA tensor, DevicePoints such
        as ScanFilter.points()); an empty cloud is a frame of zeros.  Does not wait; returns n."""
        ptr, n, stride, dev, keep = _cloud_arg(_empty_as_numpy(cloud, 3))
        if dev:
            _wait_for_producer(keep)
        _check(self.L.apdgicp_scan_ingest_histogram_add(self.h, ptr, n, stride if n else 12, dev))
        return n

    def histogram_last(self):
        """the [100] int32 counts of the last histogram_add (bin b: floor(distance) == b); waits"""
        out = np.zeros(HISTOGRAM_BINS, dtype=np.int32)
        _check(self.L.apdgicp_scan_ingest_histogram_last(self.h, _ptr(out)))
        return out

    def histogram_read(self):
        """(the [100] int64 sum of every frame since the last reset, the number of frames); waits"""
        out, frames = np.zeros(HISTOGRAM_BINS, dtype=np.int64), C.c_int64()
        _check(self.L.apdgicp_scan_ingest_histogram_read(self.h, _ptr(out), C.byref(frames)))
        return out, frames.value

    def histogram_reset(self):
        _check(self.L.apdgicp_scan_ingest_histogram_reset(self.h))

    def point_distribution(self):
        """the point_distribution command (preprocessing_nodelet.cpp:1009-1021): the sum of the frames divided by their number, element-wise,
        as integer division; zeros without a frame"""
        total, frames = self.histogram_read()
        return total // frames if frames else total

    def points(self) -> DevicePoints:
        """the rows of the last run in device memory ({x, y, z, intensity, doppler, 0, 0, 0}, 32-byte stride), valid until the next run:
        what EgoVelocityEstimator.run, ScanFilter.run, DBSCAN.run and setInputSource accept"""
        p, n = C.c_void_p(), C.c_int64()
        _check(self.L.apdgicp_scan_ingest_points(self.h, C.byref(p), None, C.byref(n)))
        return DevicePoints(p.value or 0, n.value, 32, owner=self)

    def index_device(self) -> tuple[int, int]:
        """(device pointer to one int32 per row: the point's index in the message, the number of rows)"""
        p, n = C.c_void_p(), C.c_int64()
        _check(self.L.apdgicp_scan_ingest_points(self.h, None, C.byref(p), C.byref(n)))
        return p.value or 0, n.value

    def deskew(self, cloud, ang_vel=None, scan_period: float = 0.1, T=None, intensity_column: int | None = 3) -> int:
        """cloud: [n, >=3] float32 (numpy, a torch CPU / CUDA tensor, DevicePoints such as points() or EgoVelocityEstimator.inliers());
        ang_vel: the IMU message's angular velocity (3 floats) or None (an empty IMU queue: the cloud passes through); T: 4x4 into the
        base-link frame or None.  Does not wait; returns n."""
        ptr, n, stride, dev, keep = _cloud_arg(_empty_as_numpy(cloud, 4))
        if dev:
            _wait_for_producer(keep)
        if n == 0:
            stride = 16
        ioff = -1
        if intensity_column is not None and 4 * (intensity_column + 1) <= stride:
            ioff = 4 * intensity_column
        w = np.ascontiguousarray(ang_vel, dtype=np.float64).reshape(3) if ang_vel is not None else None
        m = _mat16(T)
        self.n_deskewed = 0
        _check(self.L.apdgicp_scan_ingest_deskew(self.h, ptr, n, stride, ioff, dev, _ptr(w) if w is not None else None, float(scan_period),
                                                 _ptr(m) if m is not None else None))
        self.n_deskewed = n
        return n

    def deskewed(self) -> DevicePoints:
        """the cloud of the last deskew in device memory ({x, y, z, intensity}, 16-byte stride), valid until the next deskew.  The launch
        may still be running: synchronize() before a consumer on another stream reads it."""
        p, n = C.c_void_p(), C.c_int64()
        _check(self.L.apdgicp_scan_ingest_deskewed(self.h, C.byref(p), C.byref(n)))
        return DevicePoints(p.value or 0, n.value, 16, owner=self)

    def synchronize(self):
        _check(self.L.apdgicp_scan_ingest_synchronize(self.h))

    def to_numpy(self, which: str = "points"):
        """"points": dict(rows [n, 8] fp32, index [n] int32) of the last run; "deskewed": [n, 4] fp32 of the last deskew"""
        if which == "deskewed":
            out = np.empty((self.n_deskewed, 4), dtype=np.float32)
            if self.n_deskewed:
                _check(self.L.apdgicp_scan_ingest_deskewed_copy(self.h, _ptr(out), self.n_deskewed))
            return out
        if which != "points":
            raise KeyError(which)
        out = dict(rows=np.empty((self.n, 8), dtype=np.float32), index=np.empty(self.n, dtype=np.int32))
        if self.n:
            _check(self.L.apdgicp_scan_ingest_copy(self.h, _ptr(out["rows"]), _ptr(out["index"]), self.n))
        return out

    def stats(self) -> dict:
        """kernel launches and host waits of the last run, run_polar, deskew or histogram_add"""
        a, b = C.c_int64(), C.c_int64()
        _check(self.L.apdgicp_scan_ingest_stats(self.h, C.byref(a), C.byref(b)))
        return dict(launches=a.value, waits=b.value)


def select_imu(stamps, scan_stamp) -> tuple[int, int]:
    """deskewing's choice of the IMU message (preprocessing_nodelet.cpp:939-949) -> (index, n_erased): the first message whose stamp is
    later than the scan's, or else the last one; everything in front of the pick is erased from the queue, everything when there is no
    later message.  An empty queue: (-1, 0) -- the cloud is not deskewed (:916)."""
    n = len(stamps)
    if n == 0:
        return -1, 0
    for i in range(n):
        if stamps[i] > scan_stamp:
            return i, i
    return n - 1, n


def preprocess_scan(ingest: ScanIngest, estimator, scan_filter, xyz, intensity, doppler, registration=None, enable_dynamic_object_removal: bool = False,
                    ang_vel=None, scan_period: float = 0.1, T=None, pre_transform=None, words=None, seed: int = 0, histogram: bool = False) -> dict:
    """cloud_callback from the message to the published cloud (preprocessing_nodelet.cpp:667-830) and, with `registration`, the odometry's
    setInputSource: ingest -> EgoVelocityEstimator.run on the rows -> its inlier cloud (enable_dynamic_object_removal, :775-786) or the
    rows -> deskew + base-link transform -> ScanFilter.run -> setInputSource.  The message crosses to the device once (or is there
    already); no cloud visits the host before the filtered scan.  An empty source cloud returns before the deskew (:788-790).
    Returns dict(n_ingest, ego = the estimate, n_source, n_filtered); nothing is set when the filtered scan is empty.  histogram = True:
    the filtered scan also becomes a frame of the distance histogram (:818-828) on `ingest`."""
    n_in = ingest.run(xyz, intensity, doppler, pre_transform=pre_transform)
    rows = ingest.points()
    ego = estimator.run(rows if n_in else np.zeros((0, 5), dtype=np.float32), words=words, seed=seed)
    source = estimator.inliers() if enable_dynamic_object_removal else rows
    out = dict(n_ingest=n_in, ego=ego, n_source=source.n, n_filtered=0)
    if source.n == 0:
        return out
    _callback_tail(ingest, scan_filter, source, registration, ang_vel, scan_period, T, histogram, out)
    return out


def _callback_tail(ingest, scan_filter, source, registration, ang_vel, scan_period, T, histogram, out):
    """what the three callbacks share behind their source cloud: deskew + base-link transform, the scan filter, the distance histogram of
    the filtered scan (empty or not, as the reference pushes one), setInputSource"""
    ingest.deskew(source, ang_vel=ang_vel, scan_period=scan_period, T=T)
    ingest.synchronize()  # the scan filter runs on a stream of its own
    out["n_filtered"] = scan_filter.run(ingest.deskewed())
    if histogram:
        ingest.histogram_add(scan_filter.points() if out["n_filtered"] else np.zeros((0, 3), dtype=np.float32))
    if out["n_filtered"] and registration is not None:
        registration.setInputSource(scan_filter.points())


def preprocess_polar_scan(ingest: ScanIngest, estimator, scan_filter, targets, registration=None, ang_vel=None, scan_period: float = 0.1, T=None, words=None,
                          seed: int = 0, histogram: bool = True) -> dict:
    """cloud_callback_scan from the message to the published cloud (preprocessing_nodelet.cpp:324-464) and, with `registration`, the
    odometry's setInputSource: run_polar -> EgoVelocityEstimator.run on the rows -> ALWAYS its inlier cloud (:416-420) -> deskew +
    base-link transform -> ScanFilter.run -> the distance histogram of the filtered scan (:451-461) -> setInputSource.  `targets`: what
    ScanIngest.run_polar accepts.  A failed estimate or an empty inlier cloud returns before the deskew (:423-425).  The outlier cloud
    stays where EgoVelocityEstimator.outliers() leaves it for the RADIUS filter and DBSCAN.  Returns the dict of preprocess_scan plus
    histogram: whether a frame was added."""
    n_in = ingest.run_polar(targets)
    rows = ingest.points()
    ingest.synchronize()  # run_polar does not wait (PI2), and the estimator runs on a stream of its own
    ego = estimator.run(rows if n_in else np.zeros((0, 5), dtype=np.float32), words=words, seed=seed)
    source = estimator.inliers()
    out = dict(n_ingest=n_in, ego=ego, n_source=source.n, n_filtered=0, histogram=False)
    if not ego.success or source.n == 0:
        return out
    _callback_tail(ingest, scan_filter, source, registration, ang_vel, scan_period, T, histogram, out)
    out["histogram"] = bool(histogram)
    return out
