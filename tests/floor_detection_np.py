"""numpy restatement of the device floor detector (riv-slam_amd/csrc/apd_floor.hpp), statement by statement in the operation orders
include/apdgicp_hip.h states (section "floor plane detection and under-floor removal"), fed the same random words: the expected values of
tests/test_floor_detection.py.  Every fp32 operation is a numpy float32 operation (rounded on its own, never contracted)."""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

from ego_velocity_np import sample

F32 = np.float32
EPS = 2.220446049250313e-16
OK, FEW_POINTS, NO_MODEL, FEW_INLIERS, NOT_HORIZONTAL = range(5)


@dataclass
class Config:  # initialize_params (floor_detection_nodelet.cpp:62-70), :185, pcl::SampleConsensus, :288
    tilt_deg: float = 0.0
    sensor_height: float = 2.0
    height_clip_range: float = 1.0
    floor_pts_thresh: int = 50
    floor_normal_thresh: float = 10.0
    use_normal_filtering: bool = True
    normal_filter_thresh: float = 20.0
    floor_tolerance: float = 0.1
    distance_threshold: float = 0.06
    probability: float = 0.99
    max_iterations: int = 1000
    normal_k: int = 10
    n_hypotheses: int = 64


@dataclass
class State:  # what cloud_callback remembers (:75-80)
    prev: np.ndarray
    initialized: bool = False

    @staticmethod
    def initial(cfg: Config) -> "State":
        return State(np.array([0, 0, 0, F32(cfg.sensor_height - cfg.height_clip_range)], dtype=F32), False)


def tilt(cfg: Config):
    """(R, R^-1) in fp32: c / s evaluated in double from the fp32 angle; the inverse is the transpose"""
    angle = F32(cfg.tilt_deg * math.pi / 180.0)
    c, s = F32(math.cos(float(angle))), F32(math.sin(float(angle)))
    R = np.array([[c, 0, s], [0, (F32(1) - c) + c, 0], [-s, 0, c]], dtype=F32)
    return R, np.ascontiguousarray(R.T)


def rotate(M, xyz):
    """(r0 x + r1 y) + r2 z per coordinate"""
    x, y, z = (np.ascontiguousarray(xyz[:, q], dtype=F32) for q in range(3))
    return np.stack([(M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z for r in range(3)], axis=1)


def plane_dist(c, xyz):
    """((a x + b y) + c z) + d"""
    c = np.asarray(c, dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        return ((c[0] * xyz[:, 0] + c[1] * xyz[:, 1]) + c[2] * xyz[:, 2]) + c[3]


def clip(scan, cfg: Config):
    """:156-163 -> (mask [n], tilted [n, 4])"""
    R, _ = tilt(cfg)
    xyz = np.ascontiguousarray(scan[:, :3], dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = rotate(R, xyz)
        hi = plane_dist([0, 0, 1, F32(cfg.sensor_height + cfg.height_clip_range)], t) >= 0
        lo = plane_dist([0, 0, 1, F32(cfg.sensor_height - cfg.height_clip_range)], t) >= 0
    inten = scan[:, 3] if scan.shape[1] > 3 else np.zeros(len(scan), dtype=F32)
    return hi & ~lo, np.concatenate([t, inten[:, None].astype(F32)], axis=1)


def knn(xyz, k):
    """the k nearest points of every point, itself included: keys = (fp32 squared distance bits, index), sqdist1's arithmetic"""
    n = len(xyz)
    out = np.empty((n, k), dtype=np.int64)
    idx = np.arange(n, dtype=np.uint64)
    for a in range(0, n, 512):
        q = xyz[a:a + 512]
        d = q[:, None, :] - xyz[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        key = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx[None, :]
        part = np.argpartition(key, k - 1, axis=1)[:, :k]
        order = np.argsort(np.take_along_axis(key, part, axis=1), axis=1)
        out[a:a + 512] = np.take_along_axis(part, order, axis=1)
    return out


def normal_stat(clipped_xyz, k):
    """:280-307 as the header states it: the population covariance of the k neighbours about the query in fp64, the eigenvector of its
    smallest eigenvalue, (float)(|u_z| / |u|)"""
    xyz = np.ascontiguousarray(clipped_xyz, dtype=F32)
    nb = knn(xyz, k)
    d = xyz[nb].astype(np.float64) - xyz[:, None, :].astype(np.float64)
    mean = d.sum(axis=1) / k
    cov = np.einsum("nki,nkj->nij", d, d) / k - mean[:, :, None] * mean[:, None, :]
    _, vec = np.linalg.eigh(cov)
    u = vec[:, :, 0]
    return (np.abs(u[:, 2]) / np.sqrt((u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2])).astype(F32)


def model(p0, p1, p2):
    """SampleConsensusModelPlane::computeModelCoefficients -> (bad, [a, b, c, d] fp32)"""
    a, b = p1 - p0, p2 - p0
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        r = a / b
        if r[0] == r[1] and r[2] == r[1]:
            return True, np.zeros(4, dtype=F32)
        nx, ny, nz = a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]
        norm = np.sqrt((nx * nx + ny * ny) + nz * nz)
        nx, ny, nz = nx / norm, ny / norm, nz / norm
        d = -((nx * p0[0] + ny * p0[1]) + nz * p0[2])
    return False, np.array([nx, ny, nz, d], dtype=F32)


def inliers_of(coef, filt_xyz, thr):
    with np.errstate(invalid="ignore"):
        return np.abs(plane_dist(coef, filt_xyz)).astype(np.float64) < thr


def replay(n_in, bad, m, cfg: Config):
    """RandomSampleConsensus::computeModel over the scored hypotheses -> (iterations, skipped, winner, exhausted)"""
    it = skipped = exhausted = 0
    best, n_best, kk = -1, -(2**31 - 1), 1.0
    if m >= cfg.floor_pts_thresh and m >= 3:
        log_prob, one_over, max_skip, idx, K = math.log(1.0 - cfg.probability), 1.0 / float(m), cfg.max_iterations * 10, 0, len(n_in)
        while it < kk and skipped < max_skip:
            if idx == K:
                exhausted = 1
                break
            k = idx
            idx += 1
            if bad[k]:
                skipped += 1
                continue
            c = int(n_in[k])
            if c > n_best:
                n_best, best = c, k
                w = c * one_over
                p_no = 1.0 - (w * w) * w
                p_no = max(EPS, p_no)
                p_no = min(1.0 - EPS, p_no)
                kk = log_prob / math.log(p_no)
            it += 1
            if it > cfg.max_iterations:
                break
    return it, skipped, best, exhausted


@dataclass
class Result:
    clip_mask: np.ndarray = None
    clipped: np.ndarray = None        # [n_clipped, 4], tilted frame
    clip_src: np.ndarray = None
    stat: np.ndarray = None           # [n_clipped] or None
    nf_keep: np.ndarray = None        # [n_clipped] bool
    filtered: np.ndarray = None       # [m, 4]
    filt_src: np.ndarray = None
    ransac: bool = False
    samples: np.ndarray = None
    coef: np.ndarray = None
    bad: np.ndarray = None
    n_in: np.ndarray = None
    iterations: int = 0
    skipped: int = 0
    winner: int = -1
    exhausted: int = 0
    detected: bool = False
    reason: int = 0
    raw: np.ndarray = field(default_factory=lambda: np.zeros(4, dtype=F32))
    coeffs: np.ndarray = None         # published
    n_inliers: int = 0
    inlier_rows: np.ndarray = None
    inlier_src: np.ndarray = None
    inlier_xyzi: np.ndarray = None
    under_src: np.ndarray = None
    under_xyzi: np.ndarray = None
    initialized: bool = False


def detect(scan, cfg: Config, words, state: State, nf_keep=None) -> Result:
    """cloud_callback (:88-137) of one scan; `state` is updated in place.  nf_keep: the normal filter's decisions to use instead of the
    restatement's own (the device's, for the points whose statistic lies within the comparison's tolerance of the threshold)."""
    r = Result()
    scan = np.ascontiguousarray(scan, dtype=F32)
    K = cfg.n_hypotheses
    r.clip_mask, tilted = clip(scan, cfg)
    r.clip_src = np.flatnonzero(r.clip_mask).astype(np.int32)
    r.clipped = tilted[r.clip_mask]
    nc = len(r.clipped)
    if cfg.use_normal_filtering:
        if nc >= cfg.normal_k:
            r.stat = normal_stat(r.clipped[:, :3], cfg.normal_k)
            r.nf_keep = r.stat.astype(np.float64) > math.cos(cfg.normal_filter_thresh * math.pi / 180.0)
        else:
            r.nf_keep = np.zeros(nc, dtype=bool)
        if nf_keep is not None:
            r.nf_keep = np.asarray(nf_keep, dtype=bool)
    else:
        r.nf_keep = np.ones(nc, dtype=bool)
    _, Ri = tilt(cfg)
    kept = r.clipped[r.nf_keep]
    r.filtered = np.concatenate([rotate(Ri, kept[:, :3]), kept[:, 3:4]], axis=1) if len(kept) else np.zeros((0, 4), dtype=F32)
    r.filt_src = r.clip_src[r.nf_keep]
    m = len(r.filtered)
    r.coef, r.bad, r.n_in = np.zeros((K, 4), dtype=F32), np.zeros(K, dtype=bool), np.zeros(K, dtype=np.int32)
    r.samples = np.full((K, 3), -1, dtype=np.int32)
    r.ransac = m >= cfg.floor_pts_thresh and m >= 3
    if r.ransac:
        xyz = np.ascontiguousarray(r.filtered[:, :3])
        for k in range(K):
            s = sample(np.asarray(words[k], dtype=np.uint32), 3, m)
            r.samples[k] = s
            r.bad[k], r.coef[k] = model(xyz[s[0]], xyz[s[1]], xyz[s[2]])
            if not r.bad[k]:
                r.n_in[k] = int(inliers_of(r.coef[k], xyz, cfg.distance_threshold).sum())
    r.iterations, r.skipped, r.winner, r.exhausted = replay(r.n_in, r.bad, m, cfg)
    c = np.zeros(4, dtype=F32)
    if m < cfg.floor_pts_thresh:
        r.reason = FEW_POINTS
    elif r.winner < 0:
        r.reason = NO_MODEL
    else:
        c = r.coef[r.winner].copy()
        r.raw, r.n_inliers = c.copy(), int(r.n_in[r.winner])
        ref = Ri[:, 2]
        if r.n_inliers < cfg.floor_pts_thresh:
            r.reason = FEW_INLIERS
        elif abs(float((c[0] * ref[0] + c[1] * ref[1]) + c[2] * ref[2])) < math.cos(cfg.floor_normal_thresh * math.pi / 180.0):
            r.reason = NOT_HORIZONTAL
        elif c[2] < 0:
            c = c * F32(-1.0)
    r.detected = r.reason == OK
    if r.detected:
        state.prev, state.initialized = c.copy(), True
    r.coeffs = state.prev.copy() if state.initialized else np.array([0, 0, 1, 0], dtype=F32)
    r.initialized = state.initialized
    if r.detected:
        a = inliers_of(r.raw, r.filtered[:, :3], cfg.distance_threshold)
        r.inlier_rows = np.flatnonzero(a).astype(np.int32)
    else:
        r.inlier_rows = np.zeros(0, dtype=np.int32)
    r.inlier_src, r.inlier_xyzi = r.filt_src[r.inlier_rows], r.filtered[r.inlier_rows]
    plane = state.prev.copy()
    plane[3] = F32(np.float64(state.prev[3]) + cfg.floor_tolerance)
    with np.errstate(invalid="ignore"):
        b = plane_dist(plane, scan[:, :3]) >= 0
    r.under_src = np.flatnonzero(b).astype(np.int32)
    inten = scan[:, 3] if scan.shape[1] > 3 else np.zeros(len(scan), dtype=F32)
    r.under_xyzi = np.concatenate([scan[b, :3], inten[b, None]], axis=1)
    return r
