"""Point-to-point ICP restated in numpy: IC1 .. IC8 of include/apdgicp_hip.h, literally.  fp32 where the list says fp32 (T * p in the two
Eigen orders, the squared distance in the engine's L2_Simple order, the 4x4 product of IC6), brute-force distances, the lowest-index tie
rule, a two-pass fp64 Umeyama over numpy.linalg.svd.  `second_form_estimate` is an independent second form (scipy's cKDTree, SVD of the
demeaned data matrix product) for the self-checks of tests/test_icp.py."""
from __future__ import annotations

import numpy as np

NOT_CONVERGED, ITERATIONS, TRANSFORM, ABS_MSE, REL_MSE, NO_CORRESPONDENCES = range(6)
DBL_MAX = float(np.finfo(np.float64).max)
f32 = np.float32


def transform(T, P, linear=False):
    """IC1: T * p in fp32, pairwise (r0 x + r1 y) + (r2 z + t) or as a linear chain ((r0 x + r1 y) + r2 z) + t; non-finite rows stay."""
    T = np.asarray(T, dtype=f32)
    P = np.asarray(P, dtype=f32)
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    out = np.empty_like(P)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(3):
            a = T[r, 0] * x + T[r, 1] * y
            c = T[r, 2] * z
            out[:, r] = (a + c) + T[r, 3] if linear else a + (c + T[r, 3])
    return out


def working_cloud0(T, source, linear=False):
    """IC1: W0 = T * source, or the source itself when T is the identity."""
    T = np.asarray(T, dtype=f32)
    src = np.ascontiguousarray(source, dtype=f32)[:, :3]
    return src.copy() if np.array_equal(T, np.eye(4, dtype=f32)) else transform(T, src, linear)


def _sqdist_rows(Q, P):
    """[len(Q), len(P)] fp32 (dx dx + dy dy) + dz dz over d = Q - P (squares: the sign of d does not matter)."""
    dx = Q[:, None, 0] - P[None, :, 0]
    dy = Q[:, None, 1] - P[None, :, 1]
    dz = Q[:, None, 2] - P[None, :, 2]
    r = dx * dx
    r = r + dy * dy
    r = r + dz * dz
    return r


def nearest(Q, P, chunk=256, want_second=False):
    """For every row of Q the lowest index of its nearest row of P and that fp32 squared distance (and the second smallest distance)."""
    Q = np.asarray(Q, dtype=f32)
    P = np.asarray(P, dtype=f32)
    idx = np.empty(len(Q), dtype=np.int64)
    d2 = np.empty(len(Q), dtype=f32)
    second = np.full(len(Q), np.inf, dtype=f32)
    for a in range(0, len(Q), chunk):
        r = _sqdist_rows(P, Q[a:a + chunk]).T  # searched - query, [q, p]
        j = np.argmin(r, axis=1)  # (first occurrence: the lowest index)
        idx[a:a + chunk] = j
        d2[a:a + chunk] = r[np.arange(len(j)), j]
        if want_second and r.shape[1] > 1:
            second[a:a + chunk] = np.partition(r, 1, axis=1)[:, 1]
    return (idx, d2, second) if want_second else (idx, d2)


def correspondences(W, target, max_dist, reciprocal=False, want_second=False):
    """IC2 / IC3: (match [n] int, -1 = rejected; d2 [n] fp32 forward distance, NaN for a non-finite point; second [n])."""
    W = np.asarray(W, dtype=f32)
    tgt = np.ascontiguousarray(target, dtype=f32)[:, :3]
    n = len(W)
    valid = np.isfinite(W).all(axis=1)
    match = np.full(n, -1, dtype=np.int64)
    d2 = np.full(n, np.nan, dtype=f32)
    second = np.full(n, np.inf, dtype=f32)
    vi = np.nonzero(valid)[0]
    if len(vi) == 0:
        return (match, d2, second) if want_second else (match, d2)
    j, d, s = nearest(W[vi], tgt, want_second=True)
    d2[vi], second[vi] = d, s
    thr2 = float(max_dist) * float(max_dist)
    keep = ~(d.astype(np.float64) > thr2)
    match[vi[keep]] = j[keep]
    if reciprocal:
        js = np.unique(match[match >= 0])
        if len(js):
            back, bd = nearest(tgt[js], W[vi])  # the nearest finite point of W to target[j], lowest index
            back = vi[back]
            back_of = dict(zip(js.tolist(), zip(back.tolist(), bd.tolist())))
            for i in np.nonzero(match >= 0)[0]:
                bi, bdist = back_of[int(match[i])]
                if bi != i or float(bdist) > thr2:
                    match[i] = -1
    return (match, d2, second) if want_second else (match, d2)


def umeyama(P, Q):
    """IC5 on matched rows P (W) and Q (target), fp64, two passes: (R, t, sums[16])."""
    P = np.asarray(P, dtype=np.float64)
    Q = np.asarray(Q, dtype=np.float64)
    n = len(P)
    sp, sq = P.sum(axis=0), Q.sum(axis=0)
    pm, qm = sp / n, sq / n
    C = (Q - qm).T @ (P - pm)
    U, _, Vt = np.linalg.svd(C / n)
    S = np.diag([1.0, 1.0, 1.0 if np.linalg.det(U) * np.linalg.det(Vt) >= 0 else -1.0])
    R = U @ S @ Vt
    t = qm - R @ pm
    return R, t, sp, sq, C


def estimate(W, target, match, d2, min_corr=3):
    """IC4 / IC5: dict(T_k fp32 4x4 (identity when refused), n_corr, mse, sums, estimated, state)."""
    tgt = np.ascontiguousarray(target, dtype=f32)[:, :3]
    k = np.nonzero(match >= 0)[0]
    n = len(k)
    sums = np.zeros(16)
    out = {"T_k": np.eye(4, dtype=f32), "n_corr": n, "mse": 0.0, "sums": sums, "estimated": False, "state": NOT_CONVERGED}
    if n:
        sums[0] = d2[k].astype(np.float64).sum()
        out["mse"] = sums[0] / n
        R, t, sp, sq, C = umeyama(W[k], tgt[match[k]])
        sums[1:4], sums[4:7], sums[7:16] = sp, sq, C.reshape(9)
    if n < min_corr:
        out["state"] = NO_CORRESPONDENCES
        return out
    T = np.eye(4, dtype=f32)
    T[:3, :3] = R.astype(f32)
    T[:3, 3] = t.astype(f32)
    if not np.isfinite(T).all():
        return out
    out["T_k"], out["estimated"] = T, True
    return out


def mul4(A, B):
    """IC6: the fp32 4x4 product, each element ((a0 b0 + a1 b1) + a2 b2) + a3 b3."""
    A = np.asarray(A, dtype=f32)
    B = np.asarray(B, dtype=f32)
    out = np.empty((4, 4), dtype=f32)
    for r in range(4):
        for c in range(4):
            out[r, c] = ((A[r, 0] * B[0, c] + A[r, 1] * B[1, c]) + A[r, 2] * B[2, c]) + A[r, 3] * B[3, c]
    return out


class Criteria:
    """IC7: DefaultConvergenceCriteria.  `margins` collects |quantity / threshold - 1| of every decision made (the free-run test)."""

    def __init__(self, max_iterations, transformation_epsilon, rotation_epsilon=0.0, mse_abs=1e-12, mse_rel=-DBL_MAX, max_similar=0):
        self.max_iterations = int(max_iterations)
        self.trans_eps = float(transformation_epsilon)
        self.rot_thr = float(rotation_epsilon) if rotation_epsilon > 0 else 1.0 - float(transformation_epsilon)
        self.mse_abs, self.mse_rel, self.max_similar = float(mse_abs), float(mse_rel), int(max_similar)
        self.prev, self.similar, self.state = DBL_MAX, 0, NOT_CONVERGED
        self.margins = []

    @staticmethod
    def _rel(value, thr):
        """How far `value` is from `thr`, relative to the threshold (inf where the comparison cannot be close)."""
        if not (np.isfinite(value) and np.isfinite(thr)) or abs(thr) > 1e300:
            return np.inf
        if thr == 0:
            return np.inf if value != 0 else 0.0
        with np.errstate(over="ignore"):
            return abs(np.float64(value) / np.float64(thr) - 1.0)

    def __call__(self, iterations, T_k, mse) -> bool:
        self.state = NOT_CONVERGED
        if iterations >= self.max_iterations:
            self.state = ITERATIONS
            return True
        T = np.asarray(T_k, dtype=np.float64)
        cos = 0.5 * (T[0, 0] + T[1, 1] + T[2, 2] - 1.0)
        t2 = T[0, 3] * T[0, 3] + T[1, 3] * T[1, 3] + T[2, 3] * T[2, 3]
        # the margin of the DECISION: a conjunction that holds is as safe as its closer half, one that fails as safe as its safest failing half
        m_cos, m_t = self._rel(cos, self.rot_thr), self._rel(t2, self.trans_eps)
        if cos >= self.rot_thr and t2 <= self.trans_eps:
            self.margins.append(min(m_cos, m_t))
        else:
            self.margins.append(max(m for m, failed in ((m_cos, cos < self.rot_thr), (m_t, t2 > self.trans_eps)) if failed))
        similar = False
        if cos >= self.rot_thr and t2 <= self.trans_eps:
            if self.similar >= self.max_similar:
                self.state = TRANSFORM
                return True
            similar = True
        with np.errstate(over="ignore", invalid="ignore"):
            dabs = abs(mse - self.prev)
            drel = np.float64(dabs) / np.float64(self.prev) if self.prev != 0 else np.inf
        self.margins.append(self._rel(dabs, self.mse_abs))
        if self.mse_rel > 0:
            self.margins.append(self._rel(drel, self.mse_rel))
        if dabs < self.mse_abs:
            if self.similar >= self.max_similar:
                self.state = ABS_MSE
                return True
            similar = True
        if drel < self.mse_rel:
            if self.similar >= self.max_similar:
                self.state = REL_MSE
                return True
            similar = True
        self.similar = self.similar + 1 if similar else 0
        self.prev = mse
        return False


def iterate(W, target, max_dist, reciprocal, min_corr=3, want_second=False):
    """One iteration's IC2 .. IC5 over a given W."""
    res = correspondences(W, target, max_dist, reciprocal, want_second=want_second)
    match, d2 = res[0], res[1]
    out = estimate(W, target, match, d2, min_corr)
    out["match"], out["d2"] = match, d2
    if want_second:
        out["second"] = res[2]
    return out


def align(source, target, guess=None, max_iterations=10, transformation_epsilon=0.0, max_dist=np.sqrt(DBL_MAX), reciprocal=False,
          min_corr=3, rotation_epsilon=0.0, mse_abs=1e-12, mse_rel=-DBL_MAX, max_similar=0, linear=False, forced_T=None, want_second=False):
    """IC1 .. IC8.  forced_T: a list of 4x4 fp32 steps; iteration k then moves W and accumulates with forced_T[k] instead of its own T_k
    (teacher forcing) and runs exactly len(forced_T) iterations.  Returns dict(T, converged, iterations, state, n_matched, final_cost, W,
    trace: list of the per-iteration dicts of `iterate` + W_before, similar), margins, min_gap_ulps)."""
    g = np.eye(4, dtype=f32) if guess is None else np.asarray(guess, dtype=f32)
    W = working_cloud0(g, source, linear)
    final = g.copy()
    crit = Criteria(max_iterations, transformation_epsilon, rotation_epsilon, mse_abs, mse_rel, max_similar)
    trace, iterations, converged, state = [], 0, False, NOT_CONVERGED
    gap = np.inf
    while True:
        it = iterate(W, target, max_dist, reciprocal, min_corr, want_second)
        it["W_before"] = W
        if want_second:
            v = np.isfinite(it["d2"])
            if v.any():
                d, s = it["d2"][v], it["second"][v]
                with np.errstate(invalid="ignore"):
                    gap = min(gap, float(np.min((s - d) / np.spacing(np.maximum(d, np.finfo(f32).tiny)))))
        trace.append(it)
        if forced_T is None and not it["estimated"]:
            state = it["state"]
            it["similar"] = crit.similar
            break
        T_k = it["T_k"] if forced_T is None else np.asarray(forced_T[len(trace) - 1], dtype=f32)
        W = transform(T_k, W, linear)
        final = mul4(T_k, final)
        iterations += 1
        stop = crit(iterations, T_k, it["mse"])
        it["similar"] = crit.similar
        if forced_T is not None:
            if len(trace) == len(forced_T):
                break
            continue
        if stop:
            converged, state = True, crit.state
            break
    last = trace[-1]
    return {"T": final, "converged": converged, "iterations": iterations, "state": state, "n_matched": last["n_corr"], "final_cost": last["mse"],
            "W": W, "trace": trace, "margins": crit.margins, "min_gap_ulps": gap}


def second_form_estimate(W, target, max_dist):
    """Independent second form of IC2 + IC5 (no reciprocity): scipy's k-d tree in fp64 over the fp32 coordinates, and R from the SVD of the
    demeaned cross-covariance built with einsum.  (match, T_k fp64 4x4)."""
    from scipy.spatial import cKDTree
    W = np.asarray(W, dtype=np.float64)
    tgt = np.ascontiguousarray(target, dtype=f32)[:, :3].astype(np.float64)
    d, j = cKDTree(tgt).query(W, k=1)
    match = np.where(d * d > float(max_dist) ** 2, -1, j)
    k = match >= 0
    P, Q = W[k], tgt[match[k]]
    Pc, Qc = P - P.mean(axis=0), Q - Q.mean(axis=0)
    H = np.einsum("ni,nj->ij", Qc, Pc) / len(P)
    U, _, Vt = np.linalg.svd(H)
    D = np.eye(3)
    D[2, 2] = np.sign(np.linalg.det(U @ Vt))
    R = U @ D @ Vt
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = Q.mean(axis=0) - R @ P.mean(axis=0)
    return match, T


def ulp_close(a, b):
    """Every element of a within one fp32 ulp of b (np.spacing at the larger magnitude)."""
    a = np.asarray(a, dtype=f32)
    b = np.asarray(b, dtype=f32)
    sp = np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(f32))
    return bool(np.all(np.abs(a.astype(np.float64) - b.astype(np.float64)) <= sp.astype(np.float64)))
