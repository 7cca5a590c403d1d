"""numpy restatement of rio::RadarEgoVelocityEstimator::estimate (radar_graph_slam/src/radar_ego_velocity_estimator.cpp, "E:";
include/radar_ego_velocity_estimator.h, "EH:"), statement by statement, in the operation orders include/apdgicp_hip.h states for the
device ("Doppler ego velocity" section).  Every sum over rows is SEQUENTIAL here (np.cumsum adds one after the other): the device's
fixed-tree sums of the final fit are compared with a tolerance, everything else bit for bit.  atan2f is the fdlibm restatement of
oracle/apdgicp_np.py.  The random draws of the reference (std::random_device, E:187-194) are replaced by a caller-given [K, S] table of
uint32 words, exactly as on the device."""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

from apdgicp_np import atan2f_fdlibm

F32, F64 = np.float32, np.float64


@dataclass
class Config:
    """RadarEgoVelocityEstimatorConfig, EH:30-60 (floats there: kept as fp32 values)"""
    min_dist: float = 0.1
    max_dist: float = 400.0
    min_db: float = 5.0
    elevation_thresh_deg: float = 60.0
    azimuth_thresh_deg: float = 120.0
    doppler_velocity_correction_factor: float = 1.0
    thresh_zero_velocity: float = 0.05
    allowed_outlier_percentage: float = 0.30
    sigma_zero_velocity_x: float = 1.0e-03
    sigma_zero_velocity_y: float = 3.2e-03
    sigma_zero_velocity_z: float = 1.0e-02
    sigma_offset_radar_x: float = 0.0
    sigma_offset_radar_y: float = 0.0
    sigma_offset_radar_z: float = 0.0
    max_sigma_x: float = 0.2
    max_sigma_y: float = 0.2
    max_sigma_z: float = 0.2
    use_ransac: bool = True
    outlier_prob: float = 0.05
    success_prob: float = 0.995
    N_ransac_points: int = 5
    inlier_thresh: float = 0.5
    n_hypotheses: int = 0

    def f(self, name) -> float:
        """the field as the double an fp32 member widens to"""
        return float(F32(getattr(self, name)))


def ransac_iter(cfg: Config) -> int:
    """setRansacIter, EH:138-143"""
    if cfg.n_hypotheses:
        return int(cfg.n_hypotheses)
    return int(math.log(1.0 - cfg.f("success_prob")) / math.log(1.0 - math.pow(1.0 - cfg.f("outlier_prob"), float(F32(cfg.N_ransac_points)))))


def features(scan: np.ndarray, cfg: Config):
    """E:75-91 -> (valid mask [n], rows [n, 4] float64 of EVERY point)"""
    x, y, z, snr, dop = (np.ascontiguousarray(scan[:, q], dtype=F32) for q in range(5))
    with np.errstate(all="ignore"):
        xd, yd, zd = x.astype(F64), y.astype(F64), z.astype(F64)
        r = np.sqrt((xd * xd + yd * yd) + zd * zd)
        az = atan2f_fdlibm(y, x).astype(F64)
        rho = np.sqrt((x * x + y * y).astype(F32)).astype(F32)
        el = atan2f_fdlibm(rho, z).astype(F64) - math.pi / 2
        az_thr = cfg.f("azimuth_thresh_deg") * math.pi / 180.0
        el_thr = cfg.f("elevation_thresh_deg") * math.pi / 180.0
        valid = (r > cfg.f("min_dist")) & (r < cfg.f("max_dist")) & (snr > F32(cfg.min_db)) & (np.abs(az) < az_thr) & (np.abs(el) < el_thr)
        v = ((-dop) * F32(cfg.doppler_velocity_correction_factor)).astype(F32)
        rows = np.stack([xd / r, yd / r, zd / r, v.astype(F64)], axis=1)
    return valid, rows


def sample(words_k: np.ndarray, S: int, m: int) -> list[int]:
    """the stand-in for std::shuffle (E:194-198): S distinct rows out of m from S uint32 words"""
    picked: list[int] = []
    out = []
    for i in range(S):
        c = int(words_k[i]) % (m - i)
        for t in sorted(picked):
            if t <= c:
                c += 1
        picked.append(c)
        out.append(c)
    return out


def ldlt3(A, b):
    """the unpivoted 3x3 LDL^T of include/apdgicp_hip.h, A = (a00, a01, a02, a11, a12, a22), all float64 scalars"""
    a00, a01, a02, a11, a12, a22 = (F64(q) for q in A)
    b0, b1, b2 = (F64(q) for q in b)
    with np.errstate(all="ignore"):
        d0 = a00
        l10 = a01 / d0
        l20 = a02 / d0
        d1 = a11 - l10 * a01
        t = a12 - l20 * a01
        l21 = t / d1
        d2 = (a22 - l20 * a02) - l21 * t
        z0 = b0
        z1 = b1 - l10 * z0
        z2 = (b2 - l20 * z0) - l21 * z1
        w0, w1, w2 = z0 / d0, z1 / d1, z2 / d2
        v2 = w2
        v1 = w1 - l21 * v2
        v0 = (w0 - l10 * v1) - l20 * v2
    return np.array([v0, v1, v2], dtype=F64)


def normal_sums(rows: np.ndarray):
    """H^T H (6) and H^T y (3), added row after row"""
    h0, h1, h2, y = rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3]
    terms = [h0 * h0, h0 * h1, h0 * h2, h1 * h1, h1 * h2, h2 * h2, h0 * y, h1 * y, h2 * y]
    s = [np.cumsum(t)[-1] for t in terms]
    return s[:6], s[6:]


def abs_err(rows: np.ndarray, v: np.ndarray) -> np.ndarray:
    with np.errstate(all="ignore"):
        return np.abs(rows[:, 3] - ((rows[:, 0] * v[0] + rows[:, 1] * v[1]) + rows[:, 2] * v[2]))


def solve_full(rows: np.ndarray, cfg: Config):
    """solve3DFull(..., true), E:257-293 -> (v, sigma, sigma_in_bounds, cond(HTH))"""
    A, b = normal_sums(rows)
    v = ldlt3(A, b)
    with np.errstate(all="ignore"):
        e = ((rows[:, 0] * v[0] + rows[:, 1] * v[1]) + rows[:, 2] * v[2]) - rows[:, 3]
        ete = np.cumsum(e * e)[-1]
        a00, a01, a02, a11, a12, a22 = A
        c00, c01, c02 = a11 * a22 - a12 * a12, a02 * a12 - a01 * a22, a01 * a12 - a02 * a11
        c11, c22 = a00 * a22 - a02 * a02, a00 * a11 - a01 * a01
        det = (a00 * c00 + a01 * c01) + a02 * c02
        dof = F64(len(rows) - 3)
        sig = np.array([(ete * (c00 / det)) / dof, (ete * (c11 / det)) / dof, (ete * (c22 / det)) / dof], dtype=F64)
        ok = False
        if (sig >= 0.0).all():
            sig = np.sqrt(sig) + np.array([cfg.f("sigma_offset_radar_x"), cfg.f("sigma_offset_radar_y"), cfg.f("sigma_offset_radar_z")])
            ok = bool(sig[0] < cfg.f("max_sigma_x") and sig[1] < cfg.f("max_sigma_y") and sig[2] < cfg.f("max_sigma_z"))
    HTH = np.array([[a00, a01, a02], [a01, a11, a12], [a02, a12, a22]])
    return v, sig, ok, float(np.linalg.cond(HTH))


@dataclass
class Estimate:
    valid: np.ndarray
    rows: np.ndarray                 # [m, 4] the compacted rows
    src: np.ndarray                  # [m] index of each row in the scan
    m: int = 0
    K: int = 0
    success: bool = False
    zero_velocity: bool = False
    sigma_in_bounds: bool = False
    selected_abs_v: float = 0.0
    n0: int = 0                      # the rank of the zero-velocity test (E:104)
    v: np.ndarray = field(default_factory=lambda: np.zeros(3))
    sigma: np.ndarray = field(default_factory=lambda: np.zeros(3))
    samples: np.ndarray | None = None   # [K, S]
    v_k: np.ndarray | None = None       # [K, 3]
    n_in: np.ndarray | None = None      # [K] before the 5 % rule
    best_in: int = -1
    best_out: int = -1
    merged: bool = False
    inlier_rows: np.ndarray = field(default_factory=lambda: np.zeros(0, dtype=np.int64))
    outlier_rows: np.ndarray = field(default_factory=lambda: np.zeros(0, dtype=np.int64))
    cond: float = 0.0

    def cloud(self, scan, which="in"):
        """(xyzi [k, 4] fp32, doppler [k] fp32, source index [k]) of the inlier / outlier cloud (toRadarPointCloudType, E:41-50)"""
        r = self.inlier_rows if which == "in" else self.outlier_rows
        s = self.src[r]
        return np.ascontiguousarray(scan[s, :4], dtype=F32), (-self.rows[r, 3]).astype(F32), s.astype(np.int32)


def estimate(scan: np.ndarray, cfg: Config, words: np.ndarray | None = None) -> Estimate:
    """estimate(), E:60-170"""
    scan = np.asarray(scan, dtype=F32).reshape(-1, 5)
    valid, rows_all = features(scan, cfg)
    src = np.flatnonzero(valid)
    rows = rows_all[src]
    m = len(rows)
    K = ransac_iter(cfg) if cfg.use_ransac else 0
    out = Estimate(valid=valid, rows=rows, src=src, m=m, K=K)
    if m <= 2:                                                                       # E:99
        return out
    absv = np.abs(rows[:, 3].astype(F32))
    n0 = min(m - 1, int(float(m) * (1.0 - cfg.f("allowed_outlier_percentage"))))   # E:104 (clamped: the reference reads [m] at 0 %)
    sel = np.sort(absv.view(np.uint32))[n0:n0 + 1].view(F32)[0]                      # E:105-106 (bit order = value order for |v|)
    out.selected_abs_v, out.n0 = float(sel), n0
    thr0 = F32(cfg.thresh_zero_velocity)
    if sel < thr0:                                                                   # E:108-118
        out.zero_velocity = out.success = out.sigma_in_bounds = True
        out.sigma = np.array([cfg.f("sigma_zero_velocity_x"), cfg.f("sigma_zero_velocity_y"), cfg.f("sigma_zero_velocity_z")])
        out.inlier_rows = np.flatnonzero(absv < thr0)
        return out
    if not cfg.use_ransac:                                                           # E:138-142
        out.inlier_rows = np.arange(m)
    else:                                                                            # solve3DFullRansac, E:172-250
        S = int(cfg.N_ransac_points)
        if m < S or K == 0:                                                          # E:190, 237
            return out
        words = np.asarray(words, dtype=np.uint32).reshape(-1)[:K * S].reshape(K, S)
        thr = cfg.f("inlier_thresh")
        out.samples = np.zeros((K, S), dtype=np.int32)
        out.v_k = np.zeros((K, 3))
        out.n_in = np.zeros(K, dtype=np.int32)
        best_in_size = best_out_size = 0
        for k in range(K):
            idx = sample(words[k], S, m)
            out.samples[k] = idx
            A, b = normal_sums(rows[idx])
            v = ldlt3(A, b)
            out.v_k[k] = v
            inl = abs_err(rows, v) < thr                                             # E:203-214 (a NaN is an outlier)
            n_in = int(inl.sum())
            out.n_in[k] = n_in
            inlier_idx, outlier_idx = np.flatnonzero(inl), np.flatnonzero(~inl)
            merged = bool(F64(F32(len(outlier_idx)) / F32(m)) > 0.05)                # E:216
            if merged:
                inlier_idx, outlier_idx = np.concatenate([inlier_idx, outlier_idx]), outlier_idx[:0]
            if len(inlier_idx) > best_in_size:                                       # E:226-229
                best_in_size, out.best_in, out.inlier_rows, out.merged = len(inlier_idx), k, inlier_idx, merged
            if len(outlier_idx) > best_out_size:                                     # E:230-233
                best_out_size, out.best_out, out.outlier_rows = len(outlier_idx), k, outlier_idx
    if len(out.inlier_rows) == 0:                                                    # E:239, 248-249
        return out
    out.v, out.sigma, out.sigma_in_bounds, out.cond = solve_full(rows[out.inlier_rows], cfg)
    out.success = True                                                               # E:302
    return out
