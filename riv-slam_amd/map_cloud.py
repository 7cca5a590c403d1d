"""Map cloud generation on the GPU: radar_graph_slam::MapCloudGenerator::generate
(radar_graph_slam/src/radar_graph_slam/map_cloud_generator.cpp:13-53), which the back end runs over ALL keyframes after every graph
optimisation (radar_graph_slam_nodelet.cpp:793) and for the save-map service (:1246): every cloud transformed by its keyframe's pose in
fp32, gated at 50 m, and reduced to the occupied voxel centres of a pcl::octree::OctreePointCloud at map_cloud_resolution.  The clouds
are uploaded once per keyframe and stay on the device; a rebuild uploads poses only.  Host side of include/apdgicp_hip.h's
apdgicp_map_cloud_* entry points.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .registration import FLAG_XF_LINEAR_CHAIN, DevicePoints, _check, _cloud_arg, _ptr, load_library


class MapCloudInfo(C.Structure):
    """apdgicp_map_cloud_stats (include/apdgicp_hip.h)."""
    _fields_ = [("n_input", C.c_int64), ("n_pushed", C.c_int64), ("n_finite", C.c_int64), ("n_out", C.c_int64), ("min", C.c_double * 3), ("max", C.c_double * 3),
                ("depth", C.c_int32), ("rounds", C.c_int32), ("sort_passes", C.c_int32), ("sort_kind", C.c_int32), ("stage_ms", C.c_float * 4)]


assert C.sizeof(MapCloudInfo) == 112


class MapCloudGenerator:
    def __init__(self, device: int = 0, stream=None):
        self.L = load_library()
        self.h = C.c_void_p()
        _check(self.L.apdgicp_map_cloud_create(device, C.c_void_p(stream) if stream else None, C.byref(self.h)))
        self.n = 0
        self.n_keyframes = 0

    def __del__(self):
        try:
            if self.h:
                self.L.apdgicp_map_cloud_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def add_keyframe(self, cloud, intensity_column: int | None = 3) -> int:
        """cloud: [n, >=3] float32 {x, y, z, intensity} (numpy, a torch CPU / CUDA tensor, DevicePoints; n = 0 is allowed;
        intensity_column None or a column the cloud does not have: intensity 0).  The cloud is copied into device memory the object owns.
        Returns the keyframe's id (0, 1, 2 ...)."""
        ptr, n, stride, dev, keep = _cloud_arg(cloud)
        if dev and hasattr(keep, "data_ptr"):
            import torch
            torch.cuda.current_stream(keep.device).synchronize()  # the tensor's producer; the generator runs on a stream of its own
        if n == 0:
            stride = 16
        ioff = 4 * intensity_column if intensity_column is not None and intensity_column >= 0 and 4 * intensity_column + 4 <= stride else -1
        kid = C.c_int32(-1)
        _check(self.L.apdgicp_map_cloud_add_keyframe(self.h, ptr, n, stride, ioff, dev, C.byref(kid)))
        self.n_keyframes = kid.value + 1
        return kid.value

    def clear(self):
        """forgets every keyframe and the last result; ids start at 0 again"""
        _check(self.L.apdgicp_map_cloud_clear(self.h))
        self.n, self.n_keyframes = 0, 0

    def generate(self, poses, ids=None, resolution: float = 0.05, linear_chain: bool = False) -> int:
        """poses: one 4x4 (row-major numpy, double) per visited keyframe; ids: the keyframes to visit, in order (any subset, repeats
        allowed; default: all, in the order they were added); resolution <= 0: the transformed, gated cloud itself with its intensities
        (map_cloud_generator.cpp:38-39).  Returns the number of points of the generated cloud."""
        poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
        if ids is None:
            ids = np.arange(self.n_keyframes, dtype=np.int32)
        ids = np.ascontiguousarray(ids, dtype=np.int32).ravel()
        if len(poses) != len(ids):
            raise ValueError("one pose per keyframe")
        colmajor = np.ascontiguousarray(poses.transpose(0, 2, 1)).reshape(-1)
        n_out = C.c_int64()
        self.n = 0
        _check(self.L.apdgicp_map_cloud_generate(self.h, len(ids), _ptr(ids), _ptr(colmajor), float(resolution), FLAG_XF_LINEAR_CHAIN if linear_chain else 0,
                                                 C.byref(n_out)))
        self.n = n_out.value
        return self.n

    def points(self) -> DevicePoints:
        """the generated cloud in device memory ({x, y, z, intensity}, 16-byte stride), valid until the next generate / clear: what
        setInputTarget accepts"""
        p, n = C.c_void_p(), C.c_int64()
        _check(self.L.apdgicp_map_cloud_points(self.h, C.byref(p), C.byref(n)))
        return DevicePoints(p.value or 0, n.value, 16, owner=self)

    def to_numpy(self) -> np.ndarray:
        out = np.empty((self.n, 4), dtype=np.float32)
        if self.n:
            _check(self.L.apdgicp_map_cloud_copy(self.h, _ptr(out), self.n, 0))
        return out

    def info(self) -> dict:
        """counts (n_input, n_pushed, n_finite, n_out), the octree's depth, final box (min, max: float64[3]) and growth rounds, the sort
        (sort_passes, sort_kind: always "radix") and the device time of the last generate per stage (stage_ms: transform + gate, box
        replay, keys + sort, heads + centres)"""
        r = MapCloudInfo()
        _check(self.L.apdgicp_map_cloud_info(self.h, C.byref(r)))
        return dict(n_input=r.n_input, n_pushed=r.n_pushed, n_finite=r.n_finite, n_out=r.n_out, min=np.array(r.min, dtype=np.float64),
                    max=np.array(r.max, dtype=np.float64), depth=r.depth, rounds=r.rounds, sort_passes=r.sort_passes,
                    sort_kind="radix", stage_ms=np.array(r.stage_ms, dtype=np.float32))
