"""NDT registration (fast_gicp::NDTCuda: point-to-distribution and distribution-to-distribution) as a mode of the registration handle:
`NDT` is `registration.FastAPDGICP` with apdgicp_set_ndt switched on and the reference's setters
(fast_apdgicp/include/fast_gicp/ndt/ndt_cuda.hpp).  Semantics: the list N1 .. N9 in include/apdgicp_hip.h.  `BatchNDT` is
`registration.BatchAPDGICP` with apdgicp_batch_set_ndt switched on: many pairs at once, the optimiser loop on the device (N10 .. N15).

There is NO CPU fallback: without the HIP library or a GPU every call raises.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import registration as reg
from .registration import SOURCE, TARGET, _check, _ptr, _read_voxels, _set_fields
from .vgicp import DIRECT1, DIRECT7, DIRECT27, N_OFFSETS  # noqa: F401  NeighborSearchMethod, as the voxelized GICP mode numbers it

P2D, D2D = 0, 1          # NDTDistanceMode (ndt_settings.hpp)
DIRECT_RADIUS = 3        # refused: APDGICP_ERR_UNSUPPORTED


class NdtParams(C.Structure):
    """apdgicp_ndt_params (include/apdgicp_hip.h)."""
    _fields_ = [("resolution", C.c_double), ("distance_mode", C.c_int32), ("neighbor_search", C.c_int32)]


def default_ndt_params() -> NdtParams:
    p = NdtParams()
    reg.load_library().apdgicp_ndt_default_params(C.byref(p))
    return p


class _NdtSetters:
    """The reference's setters, enable() and enabled() over `nparams` and the `_push_mode()` / `get_ndt()` of the single or the batch class."""

    def _set(self, field: str, value):
        _set_fields(self.nparams, self._push_mode, **{field: value})

    def setDistanceMode(self, mode: int):
        self._set("distance_mode", int(mode))

    def setResolution(self, resolution: float):
        self._set("resolution", float(resolution))

    def setNeighborSearchMethod(self, method: int, radius: float = -1.0):
        """`radius` belongs to DIRECT_RADIUS, which is not offered."""
        self._set("neighbor_search", int(method))

    def enable(self):
        self._push_mode()

    def enabled(self) -> bool:
        return self.get_ndt()[1]


class NDT(_NdtSetters, reg.FastAPDGICP):
    """One registration object (== one fast_gicp::NDTCuda) on one GPU.  setInputSource / setInputTarget / swapSourceAndTarget /
    clearSource / clearTarget / align / linearize / compute_error / hasConverged / getFinalTransformation / getFitnessScore / trace are
    the base class's; align always runs the host-driven loop.  `disable()` hands the handle back to APD-GICP."""

    def __init__(self, params: reg.Params | None = None, device: int = 0, stream=None):
        super().__init__(params, device, stream)
        self.nparams = default_ndt_params()
        self._push_mode()

    def _push_mode(self):
        _check(self.L.apdgicp_set_ndt(self.h, C.byref(self.nparams)))

    def get_ndt(self):
        """(NdtParams, enabled) as the library holds them."""
        p, on = NdtParams(), C.c_int()
        _check(self.L.apdgicp_get_ndt(self.h, C.byref(p), C.byref(on)))
        return p, bool(on.value)

    def disable(self):
        """apdgicp_set_ndt(h, NULL): the handle is an APD-GICP / plain GICP object again."""
        _check(self.L.apdgicp_set_ndt(self.h, None))

    def voxel_count(self, which: int = TARGET) -> int:
        n = C.c_int64()
        _check(self.L.apdgicp_ndt_voxel_count(self.h, int(which), C.byref(n)))
        return n.value

    def voxels(self, which: int = TARGET):
        """The voxel map of SOURCE or TARGET in voxel order (ascending key): dict(coords [n,3] int32, counts [n] int32, means [n,3],
        raw [n,6] (N2: xx, yx, zx, yy, zy, zz), covs [n,3,3] (N3))."""
        return _read_voxels(lambda *a: self.L.apdgicp_ndt_get_voxels(self.h, int(which), *a), self.voxel_count(which), raw=True)

    def n_rows(self) -> int:
        """Rows of a linearize: source voxels (D2D) or source points (P2D)."""
        return self.voxel_count(SOURCE) if self.nparams.distance_mode == D2D else self.n_src

    def voxel_correspondences(self) -> np.ndarray:
        """[n_rows, n_offsets] target voxel indices of the last linearize, in offset order; -1 = miss."""
        n = self.n_rows()
        out = np.empty((n, N_OFFSETS[self.nparams.neighbor_search]), dtype=np.int32)
        _check(self.L.apdgicp_ndt_get_correspondences(self.h, _ptr(out), n))
        return out

    def build_count(self) -> int:
        """How many voxel maps this handle has built in this mode (the cache rules' test hook)."""
        n = C.c_int64()
        _check(self.L.apdgicp_ndt_build_count(self.h, C.byref(n)))
        return n.value


class BatchNDT(_NdtSetters, reg.BatchAPDGICP):
    """Many independent NDT registrations on one GPU: a batch handle with apdgicp_batch_set_ndt on (N10 .. N15).  Clouds, align,
    align_async / synchronize and fitness are the base class's, so `loop_verifier.verify_candidates(batch, ...)` takes one as it is;
    align_enqueue / align_collect raise (one batch at a time).  `disable()` hands the handle back to APD-GICP."""

    def __init__(self, params: reg.Params | None = None, device: int = 0, stream=None):
        super().__init__(params, device, stream)
        self.nparams = default_ndt_params()
        self._push_mode()

    def _push_mode(self):
        _check(self.L.apdgicp_batch_set_ndt(self.b, C.byref(self.nparams)))

    def get_ndt(self):
        """(NdtParams, enabled) as the library holds them."""
        p, on = NdtParams(), C.c_int()
        _check(self.L.apdgicp_batch_get_ndt(self.b, C.byref(p), C.byref(on)))
        return p, bool(on.value)

    def disable(self):
        _check(self.L.apdgicp_batch_set_ndt(self.b, None))

    def voxel_count(self, cloud: int) -> int:
        n = C.c_int64()
        _check(self.L.apdgicp_batch_ndt_voxel_count(self.b, int(cloud), C.byref(n)))
        return n.value

    def voxels(self, cloud: int):
        """The voxel map of cloud slot `cloud` (built if it is not current), as NDT.voxels()."""
        return _read_voxels(lambda *a: self.L.apdgicp_batch_ndt_get_voxels(self.b, int(cloud), *a), self.voxel_count(cloud), raw=True)

    def build_count(self) -> int:
        """How many NDT voxel maps this handle has built, all slots together (the cache rules' test hook)."""
        n = C.c_int64()
        _check(self.L.apdgicp_batch_ndt_build_count(self.b, C.byref(n)))
        return n.value
