"""Point-to-point ICP (pcl::IterativeClosestPoint, the ICP branch of select_registration_method(), registrations.cpp:71-78) as a mode of the
registration handle: `ICP` is `registration.FastAPDGICP` with apdgicp_set_icp switched on and PCL's setters.  Semantics: the list
IC1 .. IC10 in include/apdgicp_hip.h.  `BatchICP` is the same mode on a batch handle (IC11 .. IC16): every pair's loop runs on the device.

There is NO CPU fallback: without the HIP library or a GPU every call raises.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import registration as reg
from .registration import _check, _colmajor, _ptr

# DefaultConvergenceCriteria::ConvergenceState (apdgicp_icp_state)
NOT_CONVERGED, ITERATIONS, TRANSFORM, ABS_MSE, REL_MSE, NO_CORRESPONDENCES = range(6)
STATE_NAMES = ("NOT_CONVERGED", "ITERATIONS", "TRANSFORM", "ABS_MSE", "REL_MSE", "NO_CORRESPONDENCES")


class IcpParams(C.Structure):
    """apdgicp_icp_params (include/apdgicp_hip.h)."""
    _fields_ = [("enable", C.c_int32), ("use_reciprocal_correspondences", C.c_int32), ("min_correspondences", C.c_int32),
                ("max_similar_transforms", C.c_int32), ("euclidean_fitness_epsilon", C.c_double), ("rotation_epsilon", C.c_double),
                ("mse_threshold_absolute", C.c_double)]


def default_icp_params() -> IcpParams:
    p = IcpParams()
    reg.load_library().apdgicp_icp_default_params(C.byref(p))
    return p


def pcl_params(**kw) -> reg.Params:
    """apdgicp_params with pcl::Registration's own defaults for the fields this mode reads: 10 iterations, transformation epsilon 0, no
    gate (sqrt(DBL_MAX))."""
    p = reg.default_params()
    p.max_iterations = 10
    p.transformation_epsilon = 0.0
    p.max_correspondence_distance = float(np.sqrt(np.finfo(np.float64).max))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


class ICP(reg.FastAPDGICP):
    """One registration object (== one pcl::IterativeClosestPoint) on one GPU.  setInputSource / setInputTarget / swapSourceAndTarget /
    clearSource / clearTarget / align / hasConverged / getFinalTransformation / getFitnessScore / nearestNeighbours / transformSource are
    the base class's; setMaximumIterations, setTransformationEpsilon and setMaxCorrespondenceDistance write apdgicp_params, where
    pcl::Registration keeps them.  `params` None: PCL's defaults (pcl_params()).  `disable()` hands the handle back to APD-GICP."""

    def __init__(self, params: reg.Params | None = None, device: int = 0, stream=None):
        super().__init__(params or pcl_params(), device, stream)
        self.iparams = default_icp_params()
        self._push_icp()

    def _push_icp(self):
        _check(self.L.apdgicp_set_icp(self.h, C.byref(self.iparams)))

    def _set(self, field: str, value):
        old = getattr(self.iparams, field)
        setattr(self.iparams, field, value)
        try:
            self._push_icp()
        except reg.ApdgicpError:
            setattr(self.iparams, field, old)
            raise

    def setUseReciprocalCorrespondences(self, on: bool):
        self._set("use_reciprocal_correspondences", 1 if on else 0)

    def setEuclideanFitnessEpsilon(self, eps: float):
        self._set("euclidean_fitness_epsilon", float(eps))

    def setTransformationRotationEpsilon(self, eps: float):
        self._set("rotation_epsilon", float(eps))

    def setMinCorrespondences(self, n: int):
        self._set("min_correspondences", int(n))

    def setMaximumIterationsSimilarTransforms(self, n: int):
        self._set("max_similar_transforms", int(n))

    def setAbsoluteMSE(self, v: float):
        self._set("mse_threshold_absolute", float(v))

    def get_icp(self):
        """(IcpParams, enabled) as the library holds them."""
        p, on = IcpParams(), C.c_int()
        _check(self.L.apdgicp_get_icp(self.h, C.byref(p), C.byref(on)))
        return p, bool(on.value)

    def disable(self):
        """apdgicp_set_icp(h, NULL): the handle is an APD-GICP / plain GICP object again."""
        _check(self.L.apdgicp_set_icp(self.h, None))

    def enable(self):
        self.iparams.enable = 1
        self._push_icp()

    def enabled(self) -> bool:
        return self.get_icp()[1]

    def estimate(self, T=None):
        """The per-iteration probe (apdgicp_icp_estimate) at pose T (identity by default): dict(T_k [4, 4] float32, n_corr, mse,
        sums [16]: sum d2, sum p, sum q, then the 3x3 sum (q - qm)(p - pm)^T row-major)."""
        Tc = _colmajor(np.eye(4) if T is None else T, np.float32)
        Tk = np.zeros((4, 4), dtype=np.float32, order="F")
        n, mse, sums = C.c_int64(), C.c_double(), np.zeros(16)
        _check(self.L.apdgicp_icp_estimate(self.h, _ptr(Tc), _ptr(Tk), C.byref(n), C.byref(mse), _ptr(sums)))
        return {"T_k": np.ascontiguousarray(Tk), "n_corr": n.value, "mse": mse.value, "sums": sums}

    def correspondences(self):
        """(match, sq_dist) of the last estimate / the last iteration of the last align, in the source's order: target index or -1."""
        match = np.empty(self.n_src, dtype=np.int32)
        sqd = np.empty(self.n_src, dtype=np.float32)
        _check(self.L.apdgicp_icp_get_correspondences(self.h, _ptr(match), _ptr(sqd), self.n_src))
        return match, sqd

    def working_cloud(self) -> np.ndarray:
        """W of IC1 in the source's order, [n, 3] float32."""
        out = np.empty((self.n_src, 3), dtype=np.float32)
        _check(self.L.apdgicp_icp_get_working_cloud(self.h, _ptr(out), self.n_src))
        return out

    def trace(self):
        """dict(T_k [k, 4, 4] float32, n_corr [k], mse [k], similar [k]) of the last align, one entry per iteration."""
        n = C.c_int64()
        _check(self.L.apdgicp_icp_get_trace(self.h, 0, None, None, None, None, C.byref(n)))
        k = n.value
        Tk, nc, mse, sim = np.zeros((k, 16), dtype=np.float32), np.zeros(k, dtype=np.int64), np.zeros(k), np.zeros(k, dtype=np.int32)
        if k:
            _check(self.L.apdgicp_icp_get_trace(self.h, k, _ptr(Tk), _ptr(nc), _ptr(mse), _ptr(sim), C.byref(n)))
        return {"T_k": Tk.reshape(k, 4, 4).transpose(0, 2, 1).copy(), "n_corr": nc, "mse": mse, "similar": sim}

    def convergence_state(self) -> int:
        s = C.c_int32()
        _check(self.L.apdgicp_icp_convergence_state(self.h, C.byref(s)))
        return s.value

    def debug_counts(self):
        """(launches, waits) of the last align (tests/measure/bench_icp.py)."""
        a, b = C.c_int64(), C.c_int64()
        _check(self.L.apdgicp_icp_debug_counts(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value


def _rows(cloud) -> int:
    return int(cloud.n) if isinstance(cloud, reg.DevicePoints) else int(cloud.shape[0])


class BatchICP(reg.BatchAPDGICP):
    """Many independent point-to-point ICP registrations on one GPU: a batch handle with apdgicp_batch_set_icp on (IC11 .. IC16).  Clouds,
    align, align_async / synchronize and fitness are the base class's, so `loop_verifier.verify_candidates(batch, ...)` takes one as it is;
    align_enqueue / align_collect raise (one batch at a time).  A pair's record, state, trace, correspondences and working cloud are
    byte-identical to what `ICP` returns for the same pair.  `params` None: PCL's defaults (pcl_params()).  `disable()` hands the handle
    back to APD-GICP."""

    def __init__(self, params: reg.Params | None = None, device: int = 0, stream=None):
        super().__init__(params or pcl_params(), device, stream)
        self.iparams = default_icp_params()
        self._rows, self._last_pairs = {}, []
        self._push_icp()

    def _push_icp(self):
        _check(self.L.apdgicp_batch_set_icp(self.b, C.byref(self.iparams)))

    _set = ICP._set
    setUseReciprocalCorrespondences = ICP.setUseReciprocalCorrespondences
    setEuclideanFitnessEpsilon = ICP.setEuclideanFitnessEpsilon
    setTransformationRotationEpsilon = ICP.setTransformationRotationEpsilon
    setMinCorrespondences = ICP.setMinCorrespondences
    setMaximumIterationsSimilarTransforms = ICP.setMaximumIterationsSimilarTransforms
    setAbsoluteMSE = ICP.setAbsoluteMSE

    def _set_param(self, field: str, value):
        setattr(self.params, field, value)
        self.set_params(self.params)

    def setMaximumIterations(self, n: int):
        self._set_param("max_iterations", int(n))

    def setTransformationEpsilon(self, eps: float):
        self._set_param("transformation_epsilon", float(eps))

    def setMaxCorrespondenceDistance(self, d: float):
        self._set_param("max_correspondence_distance", float(d))

    def get_icp(self):
        """(IcpParams, enabled) as the library holds them."""
        p, on = IcpParams(), C.c_int()
        _check(self.L.apdgicp_batch_get_icp(self.b, C.byref(p), C.byref(on)))
        return p, bool(on.value)

    def disable(self):
        _check(self.L.apdgicp_batch_set_icp(self.b, None))

    def enable(self):
        self.iparams.enable = 1
        self._push_icp()

    def enabled(self) -> bool:
        return self.get_icp()[1]

    # the sizes of the slots and the pairs of the last align: what the per-pair getters size their outputs by
    def clear(self):
        super().clear()
        self._rows.clear()

    def add_cloud(self, cloud) -> int:
        idx = super().add_cloud(cloud)
        self._rows[idx] = _rows(cloud)
        return idx

    def set_cloud(self, index: int, cloud) -> int:
        idx = super().set_cloud(index, cloud)
        self._rows[idx] = _rows(cloud)
        return idx

    def set_clouds(self, first_index: int, clouds, producer_wait: bool = True):
        packed = clouds if isinstance(clouds, tuple) and clouds and clouds[0] == "packed_clouds" else self.pack_clouds(clouds)
        super().set_clouds(first_index, packed, producer_wait)
        for k in range(packed[5]):
            self._rows[first_index + k] = int(packed[2][k])

    def _remember(self, pairs):
        self._last_pairs = [(int(p.source_cloud), int(p.target_cloud)) for p in pairs] if isinstance(pairs, C.Array) else [(int(s), int(t)) for s, t in pairs]

    def align(self, pairs, guesses=None):
        self._remember(pairs)
        return super().align(pairs, guesses)

    def align_async(self, pairs, guesses=None):
        self._remember(pairs)
        return super().align_async(pairs, guesses)

    def _n_of(self, pair: int) -> int:
        if not 0 <= pair < len(self._last_pairs):
            return 0   # (the library refuses the pair)
        return self._rows.get(self._last_pairs[pair][0], 0)

    def states(self) -> np.ndarray:
        """apdgicp_icp_state of every pair of the last align, int32."""
        out = np.empty(len(self._last_pairs), dtype=np.int32)
        _check(self.L.apdgicp_batch_icp_states(self.b, _ptr(out), len(out)))
        return out

    def correspondences(self, pair: int):
        """(match, sq_dist) of the last iteration of pair `pair` of the last align, as ICP.correspondences()."""
        n = self._n_of(pair)
        match = np.empty(n, dtype=np.int32)
        sqd = np.empty(n, dtype=np.float32)
        _check(self.L.apdgicp_batch_icp_get_correspondences(self.b, int(pair), _ptr(match), _ptr(sqd), n))
        return match, sqd

    def working_cloud(self, pair: int) -> np.ndarray:
        """W of pair `pair` after the last align in the source's order, [n, 3] float32."""
        n = self._n_of(pair)
        out = np.empty((n, 3), dtype=np.float32)
        _check(self.L.apdgicp_batch_icp_get_working_cloud(self.b, int(pair), _ptr(out), n))
        return out

    def trace(self, pair: int):
        """The iterations of pair `pair` of the last align, as ICP.trace()."""
        n = C.c_int64()
        _check(self.L.apdgicp_batch_icp_get_trace(self.b, int(pair), 0, None, None, None, None, C.byref(n)))
        k = n.value
        Tk, nc, mse, sim = np.zeros((k, 16), dtype=np.float32), np.zeros(k, dtype=np.int64), np.zeros(k), np.zeros(k, dtype=np.int32)
        if k:
            _check(self.L.apdgicp_batch_icp_get_trace(self.b, int(pair), k, _ptr(Tk), _ptr(nc), _ptr(mse), _ptr(sim), C.byref(n)))
        return {"T_k": Tk.reshape(k, 4, 4).transpose(0, 2, 1).copy(), "n_corr": nc, "mse": mse, "similar": sim}

    def debug_counts(self):
        """(launches, waits, ticks) of the last align (tests/measure/bench_icp_batch.py)."""
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        _check(self.L.apdgicp_batch_icp_debug_counts(self.b, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value
