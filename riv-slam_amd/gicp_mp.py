"""fast_gicp::FastGICPMultiPoints (fast_gicp/gicp/experimental/fast_gicp_mp.hpp) as a mode of the registration handle: `FastGICPMultiPoints`
is `registration.FastAPDGICP` with apdgicp_set_gicp_mp switched on, the reference's setter names and the class's own defaults.  Semantics:
the list MP1 .. MP11 in include/apdgicp_hip.h.  The reference marks the class experimental; parity with its restatement is the bar here, not
accuracy.

There is NO CPU fallback: without the HIP library or a GPU every call raises.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import registration as reg
from .registration import _check, _ptr, _set_fields

# apdgicp_gicp_mp_state_t
NOT_CONVERGED, CONVERGED, TOO_FEW_ROWS, SINGULAR = range(4)
STATE_NAMES = ("NOT_CONVERGED", "CONVERGED", "TOO_FEW_ROWS", "SINGULAR")


class GicpMpParams(C.Structure):
    """apdgicp_gicp_mp_params (include/apdgicp_hip.h)."""
    _fields_ = [("enable", C.c_int32), ("reserved", C.c_int32), ("neighbor_search_radius", C.c_double)]


def default_gicp_mp_params() -> GicpMpParams:
    p = GicpMpParams()
    reg.load_library().apdgicp_gicp_mp_default_params(C.byref(p))
    return p


def class_params(**kw) -> reg.Params:
    """apdgicp_params with the defaults of the reference's constructor (fast_gicp_mp_impl.hpp:27-35, MP8): k 20, 64 iterations, both epsilons
    1e-5, PLANE."""
    p = reg.default_params()
    p.k_correspondences = 20
    p.max_iterations = 64
    p.rotation_epsilon = 1e-5
    p.transformation_epsilon = 1e-5
    p.regularization = reg.REG_PLANE
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


class FastGICPMultiPoints(reg.FastAPDGICP):
    """One registration object (== one fast_gicp::FastGICPMultiPoints) on one GPU.  setInputSource / setInputTarget / swapSourceAndTarget /
    clearSource / clearTarget / align / hasConverged / getFinalTransformation / getFitnessScore / linearize / getFinalHessian and
    setRotationEpsilon / setCorrespondenceRandomness / setRegularizationMethod / setNumThreads (fast_gicp_mp.hpp:44-50) are the base
    class's; `params` None: the class's defaults (class_params()).  setNeighborSearchRadius is the one extension (the reference fixes 0.5).
    `disable()` hands the handle back to APD-GICP."""

    def __init__(self, params: reg.Params | None = None, device: int = 0, stream=None):
        super().__init__(params or class_params(), device, stream)
        self.mparams = default_gicp_mp_params()
        self._push_mp()

    def _push_mp(self):
        _check(self.L.apdgicp_set_gicp_mp(self.h, C.byref(self.mparams)))

    def setNeighborSearchRadius(self, radius: float):
        _set_fields(self.mparams, self._push_mp, neighbor_search_radius=float(radius))

    def get_gicp_mp(self):
        """(GicpMpParams, enabled) as the library holds them."""
        p, on = GicpMpParams(), C.c_int()
        _check(self.L.apdgicp_get_gicp_mp(self.h, C.byref(p), C.byref(on)))
        return p, bool(on.value)

    def disable(self):
        """apdgicp_set_gicp_mp(h, NULL): the handle is an APD-GICP / plain GICP object again."""
        _check(self.L.apdgicp_set_gicp_mp(self.h, None))

    def enable(self):
        self.mparams.enable = 1
        self._push_mp()

    def enabled(self) -> bool:
        return self.get_gicp_mp()[1]

    def rows(self):
        """(row_start [n + 1] int64, index [total] int32, sq_dist [total] float32) of the last linearize, as radiusSearchOf returns them."""
        row_start = np.zeros(self.n_src + 1, dtype=np.int64)
        total = C.c_int64()
        _check(self.L.apdgicp_gicp_mp_get_rows(self.h, _ptr(row_start), self.n_src, C.byref(total)))
        idx = np.empty(total.value, dtype=np.int32)
        sqd = np.empty(total.value, dtype=np.float32)
        _check(self.L.apdgicp_gicp_mp_get_row_entries(self.h, _ptr(idx), _ptr(sqd)))
        return row_start, idx, sqd

    def fused(self):
        """dict(sum_w [n], mean_B [n, 3], cov_B [n, 6]: xx, xy, xz, yy, yz, zz) of the last linearize, in the source's order."""
        n = self.n_src
        sw, mean, cov = np.empty(n), np.empty((n, 3)), np.empty((n, 6))
        _check(self.L.apdgicp_gicp_mp_get_fused(self.h, _ptr(sw), _ptr(mean), _ptr(cov), n))
        return {"sum_w": sw, "mean_B": mean, "cov_B": cov}

    def trace(self):
        """dict(poses [k, 4, 4] the pose before each step, cost [k], n_matched [k], delta [k, 6]) of the last align."""
        n = C.c_int64()
        _check(self.L.apdgicp_gicp_mp_get_trace(self.h, 0, None, None, None, None, C.byref(n)))
        k = n.value
        poses, cost, nm, delta = np.zeros((k, 16)), np.zeros(k), np.zeros(k, dtype=np.int64), np.zeros((k, 6))
        if k:
            _check(self.L.apdgicp_gicp_mp_get_trace(self.h, k, _ptr(poses), _ptr(cost), _ptr(nm), _ptr(delta), C.byref(n)))
        return {"poses": poses.reshape(k, 4, 4).transpose(0, 2, 1).copy(), "cost": cost, "n_matched": nm, "delta": delta}

    def state(self) -> int:
        s = C.c_int32()
        _check(self.L.apdgicp_gicp_mp_state(self.h, C.byref(s)))
        return s.value

    def setProfiling(self, on: bool = True):
        """Events at the phase boundaries of the linearizes that follow (apdgicp_gicp_mp_set_profiling)."""
        _check(self.L.apdgicp_gicp_mp_set_profiling(self.h, 1 if on else 0))

    def last_phases(self):
        """dict of ms of the last profiled linearize: transform, count, scan, fill, sort, point."""
        ms = np.zeros(6)
        _check(self.L.apdgicp_gicp_mp_last_phases(self.h, _ptr(ms)))
        return dict(zip(("transform", "count", "scan", "fill", "sort", "point"), ms.tolist()))

    def debug_counts(self):
        """(launches, waits) since the start of the last align (tests/measure/bench_gicp_mp.py)."""
        a, b = C.c_int64(), C.c_int64()
        _check(self.L.apdgicp_gicp_mp_debug_counts(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value
