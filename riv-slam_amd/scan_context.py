"""Scan Context place recognition on the GPU: radar_graph_slam::SCManager (radar_graph_slam/src/radar_graph_slam/Scancontext.cpp), the
loop-candidate stage of LoopDetector::performScanContextLoopClosure (loop_detector.cpp:208).  The descriptors of all keyframes stay in
device memory; a detect call ranks the candidates by ring key, aligns by sector key, scores the cosine distance over the column shifts and
returns the best top_k -- with num_candidates = 3, search_ratio = 0.1 what SCManager computes, with num_candidates = 0, search_ratio = 1.0
exhaustive Scan Context over every candidate and every shift.  Host side of include/apdgicp_hip.h's apdgicp_scan_context_* entry points
(rules S1 .. S8 there).  detect_and_verify() hands the top_k keyframes to loop_verifier.verify_candidates.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from .registration import ApdgicpError, _check, _cloud_arg, _ptr, load_library


class ScanContextParams(C.Structure):
    """apdgicp_scan_context_params (include/apdgicp_hip.h)."""
    _fields_ = [("num_ring", C.c_int32), ("num_sector", C.c_int32), ("max_radius", C.c_double), ("azimuth_max", C.c_double), ("azimuth_min", C.c_double),
                ("num_exclude_recent", C.c_int32), ("num_candidates", C.c_int32), ("search_ratio", C.c_double), ("dist_thresh", C.c_double)]


assert C.sizeof(ScanContextParams) == 56

# apdgicp_scan_context_match
MATCH_DTYPE = np.dtype([("id", np.int32), ("shift", np.int32), ("distance", np.float64), ("ring_d2", np.float32), ("ring_rank", np.int32)])
assert MATCH_DTYPE.itemsize == 24


def default_params(**kw) -> ScanContextParams:
    p = ScanContextParams()
    _check(load_library().apdgicp_scan_context_default_params(C.byref(p)))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


@dataclass
class Detection:
    loop_id: int         # the best match's keyframe id if its distance is below dist_thresh, else -1
    yaw: float           # the best match's shift as an angle [rad] (Scancontext.cpp:374); returned, not used
    matches: np.ndarray  # MATCH_DTYPE records, best first (at most top_k)


class ScanContext:
    def __init__(self, params: ScanContextParams | None = None, device: int = 0, stream=None, **kw):
        self.L = load_library()
        self.params = params if params is not None else default_params(**kw)
        self.h = C.c_void_p()
        _check(self.L.apdgicp_scan_context_create(C.byref(self.params), device, C.c_void_p(stream) if stream else None, C.byref(self.h)))

    def __del__(self):
        try:
            if self.h:
                self.L.apdgicp_scan_context_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def set_params(self, **kw):
        """search parameters (num_exclude_recent, num_candidates, search_ratio, dist_thresh) at any time; the descriptor's geometry only
        while the database is empty"""
        p = ScanContextParams.from_buffer_copy(self.params)
        for k, v in kw.items():
            if not hasattr(p, k):
                raise AttributeError(k)
            setattr(p, k, v)
        _check(self.L.apdgicp_scan_context_set_params(self.h, C.byref(p)))
        self.params = p

    def add(self, cloud, intensity_column: int | None = 3) -> int:
        """makeAndSaveScancontextAndKeys (Scancontext.cpp:255-269).  cloud: [n, >=3] float32 {x, y, z, intensity} (numpy, a torch CPU /
        CUDA tensor, DevicePoints -- e.g. ScanFilter.points(); n = 0 gives the zero descriptor; intensity_column None or a column the cloud
        does not have: intensity 0).  Returns the descriptor's id (0, 1, 2 ...)."""
        ptr, n, stride, dev, keep = _cloud_arg(cloud)
        if dev and hasattr(keep, "data_ptr"):
            import torch
            torch.cuda.current_stream(keep.device).synchronize()  # the tensor's producer; the database runs on a stream of its own
        if n == 0:
            stride = 16
        ioff = 4 * intensity_column if intensity_column is not None and intensity_column >= 0 and 4 * intensity_column + 4 <= stride else -1
        kid = C.c_int32(-1)
        _check(self.L.apdgicp_scan_context_add(self.h, ptr, n, stride, ioff, dev, C.byref(kid)))
        return kid.value

    def add_descriptor(self, desc) -> int:
        """a ready descriptor, [num_ring, num_sector] (a saved map's); keys and norms are computed on the device"""
        d = np.ascontiguousarray(desc, dtype=np.float32)
        if d.shape != (self.params.num_ring, self.params.num_sector):
            raise ValueError("descriptor must be [num_ring, num_sector]")
        kid = C.c_int32(-1)
        _check(self.L.apdgicp_scan_context_add_descriptor(self.h, _ptr(d), C.byref(kid)))
        return kid.value

    def clear(self):
        _check(self.L.apdgicp_scan_context_clear(self.h))

    def __len__(self) -> int:
        n = C.c_int32()
        _check(self.L.apdgicp_scan_context_size(self.h, C.byref(n)))
        return n.value

    def detect(self, query_id: int, candidate_ids, top_k: int = 1) -> Detection:
        """detectLoopClosureID (Scancontext.cpp:272-379) of keyframe query_id against the candidate keyframes, in the order given"""
        ids = np.ascontiguousarray(candidate_ids, dtype=np.int32).ravel()
        k = max(1, min(int(top_k), max(len(ids), 1)))
        out = np.zeros(k, dtype=MATCH_DTYPE)
        n, loop, yaw = C.c_int32(), C.c_int32(), C.c_float()
        _check(self.L.apdgicp_scan_context_detect(self.h, int(query_id), _ptr(ids), len(ids), k, _ptr(out), C.byref(n), C.byref(loop), C.byref(yaw)))
        return Detection(loop.value, yaw.value, out[:n.value])

    def detect_batch(self, query_ids, candidate_lists, top_k: int = 1) -> list:
        """several new keyframes of one LoopDetector::detect call (loop_detector.cpp:102) in one launch sequence and one wait"""
        qids = np.ascontiguousarray(query_ids, dtype=np.int32).ravel()
        lists = [np.ascontiguousarray(c, dtype=np.int32).ravel() for c in candidate_lists]
        if len(lists) != len(qids):
            raise ValueError("one candidate list per query")
        off = np.zeros(len(qids) + 1, dtype=np.int32)
        off[1:] = np.cumsum([len(c) for c in lists])
        cand = np.concatenate(lists) if lists else np.zeros(0, dtype=np.int32)
        cand = np.ascontiguousarray(cand, dtype=np.int32)
        k = max(1, min(int(top_k), max([len(c) for c in lists] + [1])))
        out = np.zeros((len(qids), k), dtype=MATCH_DTYPE)
        n, loops, yaws = np.zeros(len(qids), dtype=np.int32), np.zeros(len(qids), dtype=np.int32), np.zeros(len(qids), dtype=np.float32)
        _check(self.L.apdgicp_scan_context_detect_batch(self.h, len(qids), _ptr(qids), _ptr(off), _ptr(cand), k, _ptr(out), _ptr(n), _ptr(loops), _ptr(yaws)))
        return [Detection(int(loops[q]), float(yaws[q]), out[q, :n[q]].copy()) for q in range(len(qids))]

    def descriptors(self, first: int = 0, count: int | None = None) -> dict:
        """reads back desc [count, R, S] float32, ring_key [count, R] float32, sector_key and col_norm [count, S] float64"""
        count = len(self) - first if count is None else count
        R, S = self.params.num_ring, self.params.num_sector
        d = dict(desc=np.zeros((count, R, S), dtype=np.float32), ring_key=np.zeros((count, R), dtype=np.float32),
                 sector_key=np.zeros((count, S), dtype=np.float64), col_norm=np.zeros((count, S), dtype=np.float64))
        _check(self.L.apdgicp_scan_context_descriptors(self.h, first, count, _ptr(d["desc"]), _ptr(d["ring_key"]), _ptr(d["sector_key"]), _ptr(d["col_norm"])))
        return d


def detect_and_verify(sc: ScanContext, batch, keyframe_clouds, new_cloud, query_id: int, candidate_ids, top_k: int = 4, fitness_score_thresh: float = 0.5):
    """Top-K Scan Context candidates into the batched geometric check: the top_k matched keyframes' clouds go to
    loop_verifier.verify_candidates unchanged (the new keyframe is the target, no initial guess: loop_detector.cpp:211 does not use the yaw).
    keyframe_clouds: indexable by keyframe id.  Returns (Loop | None, Detection, scores); Loop.candidate is the KEYFRAME id."""
    import importlib
    lv = importlib.import_module(__package__ + ".loop_verifier")
    det = sc.detect(query_id, candidate_ids, top_k)
    ids = [int(i) for i in det.matches["id"]]
    if not ids:
        return None, det, np.zeros(0)
    loop, scores, _ = lv.verify_candidates(batch, new_cloud, [keyframe_clouds[i] for i in ids], fitness_score_thresh=fitness_score_thresh)
    if loop is not None:
        loop = lv.Loop(ids[loop.candidate], loop.relative_pose, loop.fitness_score)
    return loop, det, scores
