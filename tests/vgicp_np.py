"""Restatement (test infrastructure, NOT product code) of fast_gicp::FastVGICP as include/apdgicp_hip.h pins it down in V1 .. V7:
a subclass of the APD-GICP restatement (oracle/apdgicp_np.py) that replaces update_correspondences / linearize / compute_error and
inherits step_lm, step_gn, align and calculate_covariances.  The voxel map is a plain dict filled point after point with fp64 sums
(an independent statement of V3); everything else is numpy in fp64.

Reference lines: fast_apdgicp/include/fast_gicp/gicp/impl/fast_vgicp_impl.hpp ("V:") and gicp/fast_vgicp_voxel.hpp ("VX:").
"""
from __future__ import annotations

import numpy as np

import apdgicp_np as anp

DIRECT1, DIRECT7, DIRECT27 = 0, 1, 2
ADDITIVE, ADDITIVE_WEIGHTED, MULTIPLICATIVE = 0, 1, 2
LIM = 1 << 20   # V2


def neighbor_offsets(method: int) -> np.ndarray:
    """VX:10-44, in that order."""
    if method == DIRECT1:
        return np.array([[0, 0, 0]], dtype=np.int64)
    if method == DIRECT7:
        return np.array([[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.int64)
    if method == DIRECT27:
        return np.array([[i - 1, j - 1, k - 1] for i in range(3) for j in range(3) for k in range(3)], dtype=np.int64)
    raise ValueError("unsupported neighbor search method")


def voxel_coord(x, res: float) -> np.ndarray:
    """V1 (VX:158-160): floor(x / res - 0.5) in fp64, still as doubles (the caller tests the range before it converts)."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.floor(np.asarray(x, dtype=np.float64) / float(res) - 0.5)


def build_voxelmap(target: np.ndarray, covs: np.ndarray, res: float, mode: int = ADDITIVE) -> dict:
    """V2 / V3 (VX:129-156): dict coord -> [count, mean sum, cov sum] filled in cloud order, divided by the count, numbered in
    ascending (cx, cy, cz)."""
    if mode == MULTIPLICATIVE:
        raise NotImplementedError("MULTIPLICATIVE is not offered")
    P = np.asarray(target, dtype=np.float32)[:, :3].astype(np.float64)
    C = voxel_coord(P, res)
    ok = np.isfinite(P).all(axis=1) & (np.abs(C) < LIM).all(axis=1)
    if not ok.all():
        raise ValueError(f"target point {int(np.nonzero(~ok)[0][0])} is not finite or outside the voxel key range")
    Ci = C.astype(np.int64)
    vox: dict = {}
    for i in range(P.shape[0]):
        key = (int(Ci[i, 0]), int(Ci[i, 1]), int(Ci[i, 2]))
        v = vox.get(key)
        if v is None:
            v = vox[key] = [0, np.zeros(3), np.zeros((3, 3))]
        v[0] += 1
        v[1] += P[i]          # mean += p   (VX:114)
        v[2] += covs[i]       # cov += C_B[i]  (VX:115)
    keys = sorted(vox)
    nv = len(keys)
    coords = np.array(keys, dtype=np.int32).reshape(nv, 3)
    counts = np.array([vox[k][0] for k in keys], dtype=np.int32)
    means = np.array([vox[k][1] / vox[k][0] for k in keys]).reshape(nv, 3)          # VX:119
    vcovs = np.array([vox[k][2] / vox[k][0] for k in keys]).reshape(nv, 3, 3)       # VX:120
    return {"coords": coords, "counts": counts, "means": means, "covs": vcovs, "index": {k: j for j, k in enumerate(keys)}}


def build_voxelmap_unique(target: np.ndarray, covs: np.ndarray, res: float) -> dict:
    """The same map from np.unique + np.add.at (which adds in index order): the cross-check of the dict."""
    P = np.asarray(target, dtype=np.float32)[:, :3].astype(np.float64)
    Ci = voxel_coord(P, res).astype(np.int64)
    coords, inv, counts = np.unique(Ci, axis=0, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    means = np.zeros((len(coords), 3))
    vc = np.zeros((len(coords), 3, 3))
    np.add.at(means, inv, P)
    np.add.at(vc, inv, covs)
    return {"coords": coords.astype(np.int32), "counts": counts.astype(np.int32), "means": means / counts[:, None], "covs": vc / counts[:, None, None]}


class _Empty(Exception):
    def __init__(self, T):
        self.T = T


class FastVGICP(anp.FastAPDGICP):
    def __init__(self, params: anp.Params | None = None, resolution: float = 1.0, search: int = DIRECT1, mode: int = ADDITIVE):
        super().__init__(params)
        self.resolution, self.search, self.mode = float(resolution), search, mode   # V:19-25
        self.voxelmap = None
        self.voxel_corr = None      # [n, n_offsets] voxel index, -1 = miss
        self.voxel_maha = None      # [n, n_offsets, 3, 3]
        self.n_matched = 0
        self.face_margin = np.inf       # of the last linearize
        self.face_margin_min = np.inf   # over everything since the last align() began
        self._in_align = False

    def setInputTarget(self, cloud):
        super().setInputTarget(cloud)
        self.voxelmap = None

    def _ensure(self):
        p = self.p
        if self.source_covs is None:
            self.source_covs = anp.calculate_covariances(self.source, p.k_correspondences, p.regularization)
        if self.target_covs is None:
            self.target_covs = anp.calculate_covariances(self.target, p.k_correspondences, p.regularization)
            self.voxelmap = None
        if self.voxelmap is None:
            self.voxelmap = build_voxelmap(self.target, self.target_covs, self.resolution, self.mode)

    @staticmethod
    def transform(T, a):
        """V4: q_r = ((R_r0 x + R_r1 y) + R_r2 z) + t_r in fp64"""
        T = np.asarray(T, dtype=np.float64)
        a = np.asarray(a, dtype=np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            return np.stack([((T[r, 0] * a[:, 0] + T[r, 1] * a[:, 1]) + T[r, 2] * a[:, 2]) + T[r, 3] for r in range(3)], axis=1)

    # V:73-116
    def update_correspondences(self, T):
        self._ensure()
        T = np.asarray(T, dtype=np.float64)
        offs = neighbor_offsets(self.search)
        n, no = self.source.shape[0], len(offs)
        q = self.transform(T, self.source[:, :3])
        t = voxel_coord(q, self.resolution)
        usable = np.isfinite(q).all(axis=1) & (np.abs(t) <= LIM).all(axis=1)
        corr = np.full((n, no), -1, dtype=np.int32)
        index = self.voxelmap["index"]
        rows = np.nonzero(usable)[0]
        cc = t[rows].astype(np.int64)[:, None, :] + offs[None, :, :]
        in_range = (np.abs(cc) < LIM).all(axis=2)          # V2: the range test comes first
        for a, i in enumerate(rows):
            for k in range(no):
                if in_range[a, k]:
                    corr[i, k] = index.get((int(cc[a, k, 0]), int(cc[a, k, 1]), int(cc[a, k, 2])), -1)
        # face margin: how far q / res - 0.5 is from the next integer (the offset neighbours share the fractional part)
        with np.errstate(invalid="ignore"):
            f = q[usable] / self.resolution - 0.5
            self.face_margin = float(np.abs(f - np.round(f)).min()) if usable.any() else np.inf
        self.face_margin_min = min(self.face_margin_min, self.face_margin)
        R = T[:3, :3]
        M = np.zeros((n, no, 3, 3))
        ii, kk = np.nonzero(corr >= 0)
        if len(ii):
            RCR = self.voxelmap["covs"][corr[ii, kk]] + np.einsum("ij,njk,lk->nil", R, self.source_covs[ii], R)   # V:110
            M[ii, kk] = np.linalg.inv(RCR)                                                                     # V:113
        self.voxel_corr, self.voxel_maha = corr, M
        self.n_matched = int(len(ii))
        self.correspondences = corr   # (the base class's attribute: not point indices here)

    def _cost_terms(self, T):
        ii, kk = np.nonzero(self.voxel_corr >= 0)   # point-major, offset-minor: V5's order
        v = self.voxel_corr[ii, kk]
        q = self.transform(T, self.source[ii, :3])
        e = self.voxelmap["means"][v] - q                                   # V:147
        w = np.sqrt(self.voxelmap["counts"][v].astype(np.float64))          # V:149
        M = self.voxel_maha[ii, kk]
        Me = np.einsum("nij,nj->ni", M, e)
        return q, e, w, M, Me

    # V:119-180
    def linearize(self, T, want_Hb: bool = True):
        self.trace.n_linearize += 1
        T = np.asarray(T, dtype=np.float64)
        self.update_correspondences(T)
        if self.n_matched == 0:
            if self._in_align:
                raise _Empty(T)    # V7
            return 0.0, (np.zeros((6, 6)) if want_Hb else None), (np.zeros(6) if want_Hb else None)
        q, e, w, M, Me = self._cost_terms(T)
        cost = float(np.sum(w * np.einsum("ni,ni->n", e, Me)))              # V:150
        if not want_Hb:
            return cost, None, None
        J = np.zeros((len(q), 3, 6))
        J[:, 0, 1], J[:, 0, 2] = -q[:, 2], q[:, 1]
        J[:, 1, 0], J[:, 1, 2] = q[:, 2], -q[:, 0]
        J[:, 2, 0], J[:, 2, 1] = -q[:, 1], q[:, 0]
        J[:, 0, 3] = J[:, 1, 4] = J[:, 2, 5] = -1.0                         # V:156-158
        MJ = np.einsum("nij,njk->nik", M, J)
        H = np.einsum("n,nji,njk->ik", w, J, MJ)                            # V:162
        b = np.einsum("n,nji,nj->i", w, J, Me)                              # V:163
        return cost, H, b

    # V:183-204: frozen correspondences and Mahalanobis matrices
    def compute_error(self, T) -> float:
        self.trace.n_compute_error += 1
        if self.n_matched == 0:
            return 0.0
        _, e, w, _, Me = self._cost_terms(np.asarray(T, dtype=np.float64))
        return float(np.sum(w * np.einsum("ni,ni->n", e, Me)))

    def align(self, guess=None):
        self._ensure()
        self.face_margin_min = np.inf
        self._in_align = True
        try:
            return super().align(guess)
        except _Empty as stop:     # V7: the loop stops, converged = 0, T = the pose so far
            self.converged = False
            self.final_transformation = stop.T.astype(anp.F32)
            return self.final_transformation
        finally:
            self._in_align = False
