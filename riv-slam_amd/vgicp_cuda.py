"""FAST_VGICP_CUDA (fast_gicp::FastVGICPCuda, registrations.cpp:51-61) as a mode of the registration handle: `FastVGICPCuda` is
`registration.FastAPDGICP` with apdgicp_set_vgicp_cuda switched on and the reference's setters
(fast_apdgicp/include/fast_gicp/gicp/fast_vgicp_cuda.hpp).  Semantics: the list VC1 .. VC10 in include/apdgicp_hip.h -- k fixed at 20, a
PLANE regularisation that removes line-like points from both clouds, DIRECT1 / 7 / 27 / DIRECT_RADIUS over the voxel map of what is left.
`BatchVGICPCuda` is `registration.BatchAPDGICP` with apdgicp_batch_set_vgicp_cuda switched on: per-slot prepared clouds and voxel maps and the
optimiser loop on the device (VC11 .. VC16).

There is NO CPU fallback: without the HIP library or a GPU every call that needs the device raises.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import registration as reg
from .registration import _check, _ptr, _read_voxels, _set_fields

DIRECT1, DIRECT7, DIRECT27, DIRECT_RADIUS = 0, 1, 2, 3                      # apdgicp_vgicp_cuda_params.neighbor_search
NONE, MIN_EIG, NORMALIZED_MIN_EIG, PLANE, FROBENIUS = 0, 1, 2, 3, 4         # RegularizationMethod (gicp_settings.hpp)
CPU_PARALLEL_KDTREE, GPU_BRUTEFORCE, GPU_RBF_KERNEL = 0, 1, 2               # NearestNeighborMethod
SOURCE, TARGET = reg.SOURCE, reg.TARGET


class VgicpCudaParams(C.Structure):
    """apdgicp_vgicp_cuda_params (include/apdgicp_hip.h)."""
    _fields_ = [("resolution", C.c_double), ("neighbor_search", C.c_int32), ("search_radius", C.c_double), ("regularization", C.c_int32),
                ("nn_method", C.c_int32)]


def default_vgicp_cuda_params() -> VgicpCudaParams:
    p = VgicpCudaParams()
    reg.load_library().apdgicp_vgicp_cuda_default_params(C.byref(p))
    return p


def neighbor_offsets(params: VgicpCudaParams) -> np.ndarray:
    """VC6: the offset list of `params`, [n, 3] int32 in offset order (checks the parameters; needs no handle and no device)."""
    L = reg.load_library()
    out = np.empty((257, 3), dtype=np.int32)
    n = C.c_int64()
    _check(L.apdgicp_vgicp_cuda_offsets(C.byref(params), _ptr(out), C.byref(n)))
    return out[:n.value].copy()


class _VgicpCudaSetters:
    """The reference's setters, enable(), enabled() and offsets() over `vparams` and the `_push_mode()` / `get_mode()` of the single or the batch class."""

    def _set(self, **fields):
        _set_fields(self.vparams, self._push_mode, **fields)

    def setCorrespondenceRandomness(self, k):   # VCI:38: a no-op, k is 20
        pass

    def setResolution(self, resolution: float):
        self._set(resolution=float(resolution))

    def setRegularizationMethod(self, method: int):
        self._set(regularization=int(method))

    def setNeighborSearchMethod(self, method: int, radius: float = -1.0):
        """DIRECT1 / DIRECT7 / DIRECT27, or DIRECT_RADIUS with its radius in voxels (a radius the mode does not read is not stored)."""
        if int(method) == DIRECT_RADIUS:
            self._set(neighbor_search=DIRECT_RADIUS, search_radius=float(radius))
        else:
            self._set(neighbor_search=int(method))

    def setNearestNeighborSearchMethod(self, method: int):
        self._set(nn_method=int(method))

    def enable(self):
        self._push_mode()

    def enabled(self) -> bool:
        return self.get_mode()[1]

    def offsets(self) -> np.ndarray:
        return neighbor_offsets(self.vparams)


class FastVGICPCuda(_VgicpCudaSetters, reg.FastAPDGICP):
    """One registration object (== one fast_gicp::FastVGICPCuda) on one GPU.  setInputSource / setInputTarget / swapSourceAndTarget /
    clearSource / clearTarget / align / linearize / compute_error / hasConverged / getFinalTransformation / getFitnessScore / trace are the
    base class's; align always runs the host-driven loop.  `disable()` hands the handle back to APD-GICP."""

    def __init__(self, params: reg.Params | None = None, device: int = 0, stream=None):
        super().__init__(params, device, stream)
        self.vparams = default_vgicp_cuda_params()
        self.kernel_width, self.kernel_max_dist = 0.5, 3.0   # VCI:31 (stored; only GPU_RBF_KERNEL would read them)
        self._push_mode()

    def _push_mode(self):
        _check(self.L.apdgicp_set_vgicp_cuda(self.h, C.byref(self.vparams)))

    def setKernelWidth(self, kernel_width: float, max_dist: float = -1.0):   # VCI:45-51
        self.kernel_width = float(kernel_width)
        self.kernel_max_dist = float(max_dist) if max_dist > 0.0 else 5.0 * float(kernel_width)

    def disable(self):
        """apdgicp_set_vgicp_cuda(h, NULL): the handle is an APD-GICP / plain GICP object again."""
        _check(self.L.apdgicp_set_vgicp_cuda(self.h, None))

    def get_mode(self):
        """(VgicpCudaParams, enabled) as the library holds them."""
        p, on = VgicpCudaParams(), C.c_int()
        _check(self.L.apdgicp_get_vgicp_cuda(self.h, C.byref(p), C.byref(on)))
        return p, bool(on.value)

    def kept(self, which: int) -> np.ndarray:
        """VC4: the original indices of the kept points of cloud `which`, ascending."""
        n = C.c_int64()
        _check(self.L.apdgicp_vgicp_cuda_kept(self.h, which, C.byref(n), None, 0))
        out = np.empty(n.value, dtype=np.int32)
        _check(self.L.apdgicp_vgicp_cuda_kept(self.h, which, C.byref(n), _ptr(out), n.value))
        return out

    def covariances(self, which: int):
        """(raw [n_kept, 3, 3], regularised [n_kept, 3, 3]) per kept point of cloud `which` (VC2 / VC3)."""
        n = len(self.kept(which))
        raw6, reg9 = np.empty((n, 6)), np.empty((n, 9))
        _check(self.L.apdgicp_vgicp_cuda_get_covariances(self.h, which, _ptr(raw6), _ptr(reg9), n))
        raw = raw6[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(n, 3, 3)
        return raw, reg9.reshape(n, 3, 3)

    def voxel_count(self) -> int:
        n = C.c_int64()
        _check(self.L.apdgicp_vgicp_cuda_voxel_count(self.h, C.byref(n)))
        return n.value

    def voxels(self):
        """The prepared target's voxel map in voxel order: dict(coords [n,3] int32, counts [n] int32, means [n,3], covs [n,3,3])."""
        return _read_voxels(lambda *a: self.L.apdgicp_vgicp_cuda_get_voxels(self.h, *a), self.voxel_count())

    def voxel_correspondences(self) -> np.ndarray:
        """[n_kept(source), n_offsets] voxel indices of the last linearize, in offset order; -1 = miss."""
        n = len(self.kept(SOURCE))
        out = np.empty((n, len(self.offsets())), dtype=np.int32)
        _check(self.L.apdgicp_vgicp_cuda_get_correspondences(self.h, _ptr(out), n))
        return out

    def build_count(self) -> int:
        """How many voxel maps this handle has built in this mode (the cache rules' test hook)."""
        n = C.c_int64()
        _check(self.L.apdgicp_vgicp_cuda_build_count(self.h, C.byref(n)))
        return n.value


class BatchVGICPCuda(_VgicpCudaSetters, reg.BatchAPDGICP):
    """Many independent FAST_VGICP_CUDA registrations on one GPU: a batch handle with apdgicp_batch_set_vgicp_cuda on (VC11 .. VC16): per-slot
    prepared clouds and voxel maps, the optimiser loop on the device.  Clouds, align, align_async / synchronize and fitness are the base
    class's, so `loop_verifier.verify_candidates(batch, ...)` takes one as it is; align_enqueue / align_collect raise (one batch at a time).
    `disable()` hands the handle back to APD-GICP."""

    def __init__(self, params: reg.Params | None = None, device: int = 0, stream=None):
        super().__init__(params, device, stream)
        self.vparams = default_vgicp_cuda_params()
        self._push_mode()

    def _push_mode(self):
        _check(self.L.apdgicp_batch_set_vgicp_cuda(self.b, C.byref(self.vparams)))

    def disable(self):
        _check(self.L.apdgicp_batch_set_vgicp_cuda(self.b, None))

    def get_mode(self):
        """(VgicpCudaParams, enabled) as the library holds them."""
        p, on = VgicpCudaParams(), C.c_int()
        _check(self.L.apdgicp_batch_get_vgicp_cuda(self.b, C.byref(p), C.byref(on)))
        return p, bool(on.value)

    def kept(self, cloud: int) -> np.ndarray:
        """VC4 / VC11: the original indices of the kept points of cloud slot `cloud` (prepared if it is not current), ascending."""
        n = C.c_int64()
        _check(self.L.apdgicp_batch_vgicp_cuda_kept(self.b, int(cloud), C.byref(n), None, 0))
        out = np.empty(n.value, dtype=np.int32)
        _check(self.L.apdgicp_batch_vgicp_cuda_kept(self.b, int(cloud), C.byref(n), _ptr(out), n.value))
        return out

    def covariances(self, cloud: int):
        """(raw [n_kept, 3, 3], regularised [n_kept, 3, 3]) per kept point of cloud slot `cloud` (VC2 / VC3)."""
        n = len(self.kept(cloud))
        raw6, reg9 = np.empty((n, 6)), np.empty((n, 9))
        _check(self.L.apdgicp_batch_vgicp_cuda_get_covariances(self.b, int(cloud), _ptr(raw6), _ptr(reg9), n))
        raw = raw6[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(n, 3, 3)
        return raw, reg9.reshape(n, 3, 3)

    def voxel_count(self, cloud: int) -> int:
        n = C.c_int64()
        _check(self.L.apdgicp_batch_vgicp_cuda_voxel_count(self.b, int(cloud), C.byref(n)))
        return n.value

    def voxels(self, cloud: int):
        """The voxel map over the kept points of cloud slot `cloud` (built if it is not current), as FastVGICPCuda.voxels()."""
        return _read_voxels(lambda *a: self.L.apdgicp_batch_vgicp_cuda_get_voxels(self.b, int(cloud), *a), self.voxel_count(cloud))

    def voxel_correspondences(self, pair: int) -> np.ndarray:
        """[n_kept(source), n_offsets] frozen voxel indices of pair `pair`'s last linearize in the last align, in offset order; -1 = miss."""
        n = _check(self.L.apdgicp_batch_vgicp_cuda_get_correspondences(self.b, int(pair), None, 0))
        out = np.empty((n, len(self.offsets())), dtype=np.int32)
        _check(self.L.apdgicp_batch_vgicp_cuda_get_correspondences(self.b, int(pair), _ptr(out), n))
        return out

    def build_count(self):
        """(clouds prepared, maps built) by this handle in this mode, all slots together (the cache rules' test hook)."""
        p, m = C.c_int64(), C.c_int64()
        _check(self.L.apdgicp_batch_vgicp_cuda_build_count(self.b, C.byref(p), C.byref(m)))
        return p.value, m.value

    def debug_counts(self):
        """(host waits spent preparing clouds, host waits spent building maps, both since the handle was created; ticks of the last align)."""
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        _check(self.L.apdgicp_batch_vgicp_cuda_debug_counts(self.b, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def last_phases(self):
        """(preparation, map builds, ticks) of the last align in ms by the host clock; meaningful after set_profiling(True)."""
        ms = (C.c_double * 3)()
        _check(self.L.apdgicp_batch_vgicp_cuda_last_phases(self.b, ms))
        return tuple(ms)
