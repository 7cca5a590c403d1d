"""Voxelized GICP (fast_gicp::FastVGICP, the FAST_VGICP branch of select_registration_method(), registrations.cpp:62-70) as a mode of
the registration handle: `FastVGICP` is `registration.FastAPDGICP` with apdgicp_set_vgicp switched on and the reference's three setters
(fast_apdgicp/include/fast_gicp/gicp/fast_vgicp.hpp).  Semantics: the list V1 .. V7 in include/apdgicp_hip.h.  `BatchVGICP` is
`registration.BatchAPDGICP` with apdgicp_batch_set_vgicp switched on: per-slot voxel maps and the optimiser loop on the device (V8 .. V12).

There is NO CPU fallback: without the HIP library or a GPU every call raises.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import registration as reg
from .registration import _check, _ptr, _read_voxels, _set_fields

DIRECT1, DIRECT7, DIRECT27 = 0, 1, 2                    # NeighborSearchMethod (gicp_settings.hpp)
ADDITIVE, ADDITIVE_WEIGHTED, MULTIPLICATIVE = 0, 1, 2   # VoxelAccumulationMode
N_OFFSETS = {DIRECT1: 1, DIRECT7: 7, DIRECT27: 27}


class VgicpParams(C.Structure):
    """apdgicp_vgicp_params (include/apdgicp_hip.h)."""
    _fields_ = [("resolution", C.c_double), ("neighbor_search", C.c_int32), ("voxel_mode", C.c_int32)]


def default_vgicp_params() -> VgicpParams:
    p = VgicpParams()
    reg.load_library().apdgicp_vgicp_default_params(C.byref(p))
    return p


class _VgicpSetters:
    """The reference's three setters and enable() over `vparams` and the `_push_mode()` of the single or the batch class."""

    def _set(self, field: str, value):
        _set_fields(self.vparams, self._push_mode, **{field: value})

    def setResolution(self, resolution: float):
        self._set("resolution", float(resolution))

    def setNeighborSearchMethod(self, method: int):
        self._set("neighbor_search", int(method))

    def setVoxelAccumulationMode(self, mode: int):
        self._set("voxel_mode", int(mode))

    def enable(self):
        self._push_mode()


class FastVGICP(_VgicpSetters, reg.FastAPDGICP):
    """One registration object (== one fast_gicp::FastVGICP) on one GPU.  setInputSource / setInputTarget / align / linearize /
    compute_error / hasConverged / getFinalTransformation / getFitnessScore / trace are the base class's; align always runs the
    host-driven loop.  `disable()` hands the handle back to APD-GICP."""

    def __init__(self, params: reg.Params | None = None, device: int = 0, stream=None):
        super().__init__(params, device, stream)
        self.vparams = default_vgicp_params()
        self._push_mode()

    def _push_mode(self):
        _check(self.L.apdgicp_set_vgicp(self.h, C.byref(self.vparams)))

    def disable(self):
        """apdgicp_set_vgicp(h, NULL): the handle is an APD-GICP / plain GICP object again."""
        _check(self.L.apdgicp_set_vgicp(self.h, None))

    def enabled(self) -> bool:
        on = C.c_int()
        _check(self.L.apdgicp_get_vgicp(self.h, None, C.byref(on)))
        return bool(on.value)

    def voxel_count(self) -> int:
        n = C.c_int64()
        _check(self.L.apdgicp_vgicp_voxel_count(self.h, C.byref(n)))
        return n.value

    def voxels(self):
        """The target's voxel map in voxel order (ascending key): dict(coords [n,3] int32, counts [n] int32, means [n,3], covs [n,3,3])."""
        return _read_voxels(lambda *a: self.L.apdgicp_vgicp_get_voxels(self.h, *a), self.voxel_count())

    def voxel_correspondences(self) -> np.ndarray:
        """[n_source, n_offsets] voxel indices of the last linearize, in offset order; -1 = miss."""
        out = np.empty((self.n_src, N_OFFSETS[self.vparams.neighbor_search]), dtype=np.int32)
        _check(self.L.apdgicp_vgicp_get_correspondences(self.h, _ptr(out), self.n_src))
        return out

    def build_count(self) -> int:
        """How many voxel maps this handle has built (the cache rules' test hook)."""
        n = C.c_int64()
        _check(self.L.apdgicp_vgicp_build_count(self.h, C.byref(n)))
        return n.value


class BatchVGICP(_VgicpSetters, reg.BatchAPDGICP):
    """Many independent voxelized-GICP registrations on one GPU: a batch handle with apdgicp_batch_set_vgicp on (V8 .. V12).  Clouds, align,
    align_async / synchronize and fitness are the base class's, so `loop_verifier.verify_candidates(batch, ...)` takes one as it is;
    align_enqueue / align_collect raise (one batch at a time).  `disable()` hands the handle back to APD-GICP."""

    def __init__(self, params: reg.Params | None = None, device: int = 0, stream=None):
        super().__init__(params, device, stream)
        self.vparams = default_vgicp_params()
        self._push_mode()

    def _push_mode(self):
        _check(self.L.apdgicp_batch_set_vgicp(self.b, C.byref(self.vparams)))

    def get_vgicp(self):
        """(VgicpParams, enabled) as the library holds them."""
        p, on = VgicpParams(), C.c_int()
        _check(self.L.apdgicp_batch_get_vgicp(self.b, C.byref(p), C.byref(on)))
        return p, bool(on.value)

    def disable(self):
        _check(self.L.apdgicp_batch_set_vgicp(self.b, None))

    def enabled(self) -> bool:
        return self.get_vgicp()[1]

    def voxel_count(self, cloud: int) -> int:
        n = C.c_int64()
        _check(self.L.apdgicp_batch_vgicp_voxel_count(self.b, int(cloud), C.byref(n)))
        return n.value

    def voxels(self, cloud: int):
        """The voxel map of cloud slot `cloud` (built if it is not current), as FastVGICP.voxels()."""
        return _read_voxels(lambda *a: self.L.apdgicp_batch_vgicp_get_voxels(self.b, int(cloud), *a), self.voxel_count(cloud))

    def build_count(self) -> int:
        """How many voxel maps this handle has built, all slots together (the cache rules' test hook)."""
        n = C.c_int64()
        _check(self.L.apdgicp_batch_vgicp_build_count(self.b, C.byref(n)))
        return n.value
