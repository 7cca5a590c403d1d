"""Restatement of FastGICPMultiPoints as a mode of the registration handle (MP1 .. MP11 of include/apdgicp_hip.h), in numpy, fp64.

Literal: the rows come from the dense key matrix of tests/search_np.py (nothing here knows how the device walks the target), and MP4 .. MP7
are written out statement by statement -- elementwise over the points, never through a matrix product whose summation order numpy chooses.
The covariances are INPUTS (the device's own, MP1): this file restates what the mode does with them, not how they are estimated.
Per point the arithmetic is in the device's written order; the sums over the points are numpy's, which is why H, g and the cost are compared
by tolerance and the fused terms almost bit for bit.
"""
import math

import numpy as np

import apdgicp_np as anp
import search_np

F32 = np.float32
NOT_CONVERGED, CONVERGED, TOO_FEW_ROWS, SINGULAR = range(4)


def sym6(C):
    """[n, 3, 3] (or [n, 4, 4]) -> the six unique entries xx, xy, xz, yy, yz, zz as [n, 6]"""
    C = np.asarray(C, dtype=np.float64)
    return np.stack([C[:, 0, 0], C[:, 0, 1], C[:, 0, 2], C[:, 1, 1], C[:, 1, 2], C[:, 2, 2]], axis=1)


def queries(T, source, linear=False):
    """MP2: q_i = T_f * p_i in fp32"""
    return anp.transform_points_f32(np.asarray(T, dtype=np.float64), np.asarray(source, dtype=F32), linear)


def rows(q, target, radius):
    """MP3: (row_start, index, sq_dist); a non-finite query has an empty row (its distances are not below r2)"""
    with np.errstate(invalid="ignore", over="ignore"):
        return search_np.radius_search(q, np.asarray(target, dtype=F32), radius, 0)


def weight(d2, radius):
    """MP4: the square root in fp32, the division in fp64"""
    s = np.sqrt(np.asarray(d2, dtype=F32))
    assert s.dtype == F32
    return np.maximum(1e-3, np.minimum(1.0, 1.0 - s.astype(np.float64) / np.float64(radius)))


def fuse(row_start, index, sq_dist, target, cov_t6, radius):
    """MP4: (sum_w [n], mean_B [n, 3], cov_B [n, 6]) in row order, sums started at 0.0; zeros for an empty row"""
    n = len(row_start) - 1
    lens = np.diff(row_start)
    t64 = np.asarray(target, dtype=F32).astype(np.float64)
    sw, sm, sc = np.zeros(n), np.zeros((n, 3)), np.zeros((n, 6))
    for e in range(int(lens.max()) if n else 0):   # entry e of every row that has one: each row is summed in its own order
        act = np.nonzero(lens > e)[0]
        at = row_start[act] + e
        w = weight(sq_dist[at], radius)
        j = index[at]
        sw[act] = sw[act] + w
        sm[act] = sm[act] + w[:, None] * t64[j]
        sc[act] = sc[act] + w[:, None] * cov_t6[j]
    ok = lens > 0
    mean, cov = np.zeros((n, 3)), np.zeros((n, 6))
    mean[ok] = sm[ok] / sw[ok, None]
    cov[ok] = sc[ok] / sw[ok, None]
    return sw, mean, cov


def _rotate(R, c):
    """R C R^T for the six unique entries (columns of c), written as the device writes it"""
    xx, xy, xz, yy, yz, zz = (c[:, k] for k in range(6))
    rc = [[R[i, 0] * xx + R[i, 1] * xy + R[i, 2] * xz, R[i, 0] * xy + R[i, 1] * yy + R[i, 2] * yz, R[i, 0] * xz + R[i, 1] * yz + R[i, 2] * zz] for i in range(3)]
    row = lambda i, j: rc[i][0] * R[j, 0] + rc[i][1] * R[j, 1] + rc[i][2] * R[j, 2]
    return row(0, 0), row(0, 1), row(0, 2), row(1, 1), row(1, 2), row(2, 2)


def _inverse(xx, xy, xz, yy, yz, zz):
    """the 3x3 inverse by cofactors"""
    c00 = yy * zz - yz * yz
    c01 = yz * xz - xy * zz
    c02 = xy * yz - yy * xz
    det = xx * c00 + xy * c01 + xz * c02
    i = 1.0 / det
    return c00 * i, c01 * i, c02 * i, (xx * zz - xz * xz) * i, (xy * xz - xx * yz) * i, (xx * yy - xy * xy) * i


def residuals(T, source, cov_s6, mean_B, cov_B, ok, M=None):
    """MP5 per point with a non-empty row: (l [m, 3], J [m, 3, 6], M six columns).  `M` given: frozen (the Jacobian test)."""
    T = np.asarray(T, dtype=np.float64)
    R, t = T[:3, :3], T[:3, 3]
    a = np.asarray(source, dtype=F32)[ok].astype(np.float64)
    Ta = [((R[i, 0] * a[:, 0] + R[i, 1] * a[:, 1]) + R[i, 2] * a[:, 2]) + t[i] for i in range(3)]
    d = [mean_B[ok][:, i] - Ta[i] for i in range(3)]
    with np.errstate(all="ignore"):
        if M is None:
            rot = _rotate(R, cov_s6[ok])
            M = _inverse(*(cov_B[ok][:, k] + rot[k] for k in range(6)))
        xx, xy, xz, yy, yz, zz = M
        Mr = [[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]]
        l = np.stack([(Mr[i][0] * d[0] + Mr[i][1] * d[1]) + Mr[i][2] * d[2] for i in range(3)], axis=1)
        tx, ty, tz = Ta
        J = np.empty((len(a), 3, 6))
        for i in range(3):   # M * [skew(Ta) | -I]
            J[:, i, 0] = Mr[i][1] * tz - Mr[i][2] * ty
            J[:, i, 1] = Mr[i][2] * tx - Mr[i][0] * tz
            J[:, i, 2] = Mr[i][0] * ty - Mr[i][1] * tx
            J[:, i, 3], J[:, i, 4], J[:, i, 5] = -Mr[i][0], -Mr[i][1], -Mr[i][2]
    return l, J, M


def linearize(T, source, target, cov_s, cov_t, radius, linear=False):
    """MP2 .. MP5 at T: dict(H, g, cost, n_matched, rows, sum_w, mean_B, cov_B)"""
    cov_s6, cov_t6 = sym6(cov_s), sym6(cov_t)
    rs, idx, d2 = rows(queries(T, source, linear), target, radius)
    sw, mean, cov = fuse(rs, idx, d2, target, cov_t6, radius)
    ok = np.diff(rs) > 0
    l, J, _ = residuals(T, source, cov_s6, mean, cov, ok)
    with np.errstate(all="ignore"):
        H = np.zeros((6, 6))
        for a in range(6):
            for b in range(6):
                H[a, b] = np.sum((J[:, 0, a] * J[:, 0, b] + J[:, 1, a] * J[:, 1, b]) + J[:, 2, a] * J[:, 2, b])
        g = np.array([np.sum((J[:, 0, a] * l[:, 0] + J[:, 1, a] * l[:, 1]) + J[:, 2, a] * l[:, 2]) for a in range(6)])
        cost = float(np.sum((l[:, 0] * l[:, 0] + l[:, 1] * l[:, 1]) + l[:, 2] * l[:, 2]))
    return {"H": H, "g": g, "cost": cost, "n_matched": int(ok.sum()), "rows": (rs, idx, d2), "sum_w": sw, "mean_B": mean, "cov_B": cov}


def solve(H, g):
    """MP6: H delta = g by the 6x6 LDL^T without pivoting of the host loop (a vanishing pivot zeroes its unknown)"""
    L = [[0.0] * 6 for _ in range(6)]
    D = [0.0] * 6
    with np.errstate(all="ignore"):
        for j in range(6):
            dj = np.float64(H[j, j])
            for k in range(j):
                dj = dj - L[j][k] * L[j][k] * D[k]
            D[j] = dj
            inv = 1.0 / dj if abs(dj) > 1e-300 else 0.0
            for i in range(j + 1, 6):
                v = np.float64(H[i, j])
                for k in range(j):
                    v = v - L[i][k] * L[j][k] * D[k]
                L[i][j] = v * inv
        y = [0.0] * 6
        for i in range(6):
            v = np.float64(g[i])
            for k in range(i):
                v = v - L[i][k] * y[k]
            y[i] = v
        for i in range(6):
            y[i] = y[i] / D[i] if abs(D[i]) > 1e-300 else 0.0
        x = [0.0] * 6
        for i in range(5, -1, -1):
            v = np.float64(y[i])
            for k in range(i + 1, 6):
                v = v - L[k][i] * x[k]
            x[i] = v
    return np.array(x, dtype=np.float64)


def update(T, delta):
    """MP6: R <- so3_exp(-delta_r) R, t <- t - delta_t (the translation is not rotated)"""
    T = np.asarray(T, dtype=np.float64)
    E = anp.so3_exp(-np.asarray(delta[:3], dtype=np.float64))
    out = np.eye(4)
    for i in range(3):
        for j in range(3):
            out[i, j] = (E[i, 0] * T[0, j] + E[i, 1] * T[1, j]) + E[i, 2] * T[2, j]
        out[i, 3] = T[i, 3] - delta[3 + i]
    return out


def deciding(delta, rot_eps, trans_eps):
    """MP7: max(|so3_exp(delta_r) - I| / rot_eps, |delta_t| / trans_eps); converged iff it is below 1 (NaN: not converged)"""
    with np.errstate(all="ignore"):
        Rd = np.abs(anp.so3_exp(np.asarray(delta[:3], dtype=np.float64)) - np.eye(3)) * (1.0 / rot_eps)
        td = np.abs(np.asarray(delta[3:], dtype=np.float64)) * (1.0 / trans_eps)
    v = np.concatenate([Rd.ravel(), td])
    return float("nan") if np.isnan(v).any() else float(v.max())


def align(source, target, cov_s, cov_t, radius, guess=None, max_iterations=64, rot_eps=1e-5, trans_eps=1e-5, linear=False):
    """MP7, free running: dict(T [4, 4] float32, state, converged, iterations, n_linearize, n_matched, final_cost, deciding [per iteration],
    poses, costs, deltas)"""
    T = np.eye(4) if guess is None else np.asarray(guess, dtype=F32).astype(np.float64)
    T[3] = (0.0, 0.0, 0.0, 1.0)
    out = {"state": NOT_CONVERGED, "converged": False, "iterations": 0, "n_linearize": 0, "n_matched": 0, "final_cost": 0.0, "deciding": [], "poses": [], "costs": [],
           "deltas": []}
    for it in range(max_iterations):
        out["iterations"] = it
        lin = linearize(T, source, target, cov_s, cov_t, radius, linear)
        out["n_linearize"] += 1
        out["n_matched"], out["final_cost"] = lin["n_matched"], lin["cost"]
        out["poses"].append(T.copy()), out["costs"].append(lin["cost"])
        if lin["n_matched"] < 2:
            out["state"] = TOO_FEW_ROWS
            out["deltas"].append(np.zeros(6))
            break
        delta = solve(lin["H"], lin["g"])
        out["deltas"].append(delta)
        if not np.isfinite(delta).all():
            out["state"] = SINGULAR
            break
        T = update(T, delta)
        q = deciding(delta, rot_eps, trans_eps)
        out["deciding"].append(q)
        if not math.isnan(q) and q < 1.0:
            out["converged"], out["state"] = True, CONVERGED
            break
    out["T"] = T.astype(F32)
    return out
